// scorer_tuning.h -- everything a build of the interval scorer, the projection GEMMs or the three-limb split may vary with -D,
// each with its meaning and default (the sweep kernel's counterpart: persist_tuning.h).  What is left are probe builds and
// timing ablations that a script under tools/ drives (tools/README.md lists the recipes, tests/test_abi.py compiles them).
// The schedules that were measured neutral or slower are no longer in the source; the sentence that records each measurement
// stands where the surviving form is (and in DESIGN.md section 3), their code is in git history (last at commit b09adaa):
//   SEMICRF_SCORE_PRIO, SEMICRF_SCORE_XNS, SEMICRF_SCORE_SCHED3, SEMICRF_SCORE_DEBUG (run time)   scorer_fwd_tile_ref.h, _tile3.h
//   SEMICRF_TILED_PINGPONG, SEMICRF_TILED_SPREAD                                                   scorer_tiled.hip
//   SEMICRF_GEMM_SPREAD, SEMICRF_PACK_ORDER                                                        scorer_bwd_gemm_exact.h, _pack.h
//   SEMICRF_G3_{INTERLEAVE,PHASED,FINE,LEAD,PRIO_FLIP,FILL_LOADS,MMA_ORDER,DRAIN,DBG}, SEMICRF_MMA_PRIO     scorer_bwd_gemm3.h
//   SEMICRF_P3_MMA_ORDER, SEMICRF_P3_PHASED, SEMICRF_MMA_PRIO                                      proj_gemm3.hip
//   SEMICRF_SPLIT_SCALAR_SUB                                                                       bf16x3.h
#pragma once

// ---- forward ---------------------------------------------------------------------------------------------------------------------
// SEMICRF_SCORE_PROBE (defined or not; tools/score_probe.py): interval_score_tile3_kernel writes one wave's cycle accounting --
// [0] waiting at the barrier, [1] operand reads + matrix instructions + split + limb stores, [2] the fetch of the chunk after next,
// [3] the epilogue -- over the unused cells S[0, 1.., :] of a lower-triangle-only launch.  Results stay right; the kernel is slower.
//
// SEMICRF_TILED_PROBE (defined or not; tools/tiled_probe.py): the same for interval_score_tiled_kernel -- 0 operand wait + barrier,
// 1 stores, 2 requests, 4 contraction, 7 the rest.

// ---- backward, three-limb GEMMs (scorer_bwd_gemm3.h) ------------------------------------------------------------------------------
#ifndef SEMICRF_G3_PROBE
#define SEMICRF_G3_PROBE 0        // 1: cycle accounting of every wave instead of results (tools/bwd3_probe.py --probe): [0] multiply, [1] epilogue,
#endif                            // [2] the barrier, [3] wait for the set's loads, [5] requests; 2: one stamp at each end of a wave's life only
#ifndef SEMICRF_G3_ABL
#define SEMICRF_G3_ABL 0          // timing ablations (tools/bwd3_probe.py; variant builds only; results are wrong): 1 no split pieces,
#endif                            // 2 the operands of a chunk's first instruction group for all of it (no LDS reads inside), 4 no requests

// ---- projection, three-limb GEMM (proj_gemm3.hip) ---------------------------------------------------------------------------------
#ifndef SEMICRF_P3_PROBE
#define SEMICRF_P3_PROBE 0        // 1: per-wave cycle accounting in place of the first output rows (tools/bwd3_probe.py --proj-probe)
#endif
