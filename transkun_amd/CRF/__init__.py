# mirrors /root/reference/transkun/CRF/__init__.py:1
from .NeuralSemiCRFInterval import *  # noqa: F401,F403
from .NeuralSemiCRFInterval import (NeuralSemiCRFInterval, viterbi, viterbiBackward, computeLogZ,  # noqa: F401
                                    forward_backward, evalPath, computeLogZFasterGrad,
                                    ComputeLogZFasterGrad, sample, sample_packed,
                                    viterbi_nbest, viterbi_nbest_packed, Posteriors, posteriors,
                                    interval_marginals, interval_marginals_packed,
                                    decode_marginal, decode_marginal_packed,
                                    decode_mbr, decode_mbr_packed,
                                    expectation, entropy, covariance,
                                    PathStats, compare_paths, compare_paths_packed, decode_stats)
