#pragma once
// persist_tuning.h -- everything about the persistent sweep (persist.hip) that a build can vary with -D.
//
// Tuned numbers: each is the measured-best value (DESIGN.md section 3 has the measurements); a variant library is
// `python tools/mkvar.py NAME DEFINE=V ...`.  Structural alternatives that were measured neutral or slower (near tiles, two
// spines per workgroup, two loader waves, the loader / far-wave ablations) are not selectable: their code is gone.

// ---- probe builds (tools/*_trace.py, activity_hist.py, clock_probe.py, realmath_probe.py): never in the release library --------
#ifndef SEMICRF_PANEL_PROBES
#define SEMICRF_PANEL_PROBES 0      // 1: keep the panel timing probes (debug flags 4 and 32) in the hot loop
#endif
#ifndef SEMICRF_PROBE_TASKS
#define SEMICRF_PROBE_TASKS 0      // 1 (with SEMICRF_PANEL_PROBES): the task timeline of tools/task_trace.py (its own build: registers)
#endif
#ifndef SEMICRF_PROBE_HIST
#define SEMICRF_PROBE_HIST 0       // 1 (with SEMICRF_PANEL_PROBES): the per-tile activity histogram of tools/activity_hist.py (spills: its own build)
#endif
#ifndef SEMICRF_CT_DBG
#define SEMICRF_CT_DBG -1          // >= 0 (with SEMICRF_PANEL_PROBES=1): the debug flags as a compile-time constant -- a timing ablation
#endif                              // without the probe build's register pressure (the flags' dead branches fold away)
// (SEMICRF_DEBUG_BUILD=1: the launch-geometry knobs are read from the environment, see read_knobs in persist.hip)

// ---- workgroup and spine -------------------------------------------------------------------------------------------------------
#ifndef SEMICRF_NT
#define SEMICRF_NT 640              // threads per workgroup (10 waves: a spine workgroup = 4 ring + loader + far + 4 spare waves)
#endif
#ifndef SEMICRF_RING
#define SEMICRF_RING 4              // waves per ring; band = RING-1 off-diagonal blocks + the diagonal block
#endif
#ifndef SEMICRF_NRBUF
#define SEMICRF_NRBUF 4             // row-block buffers between the loader and the ring
#endif
#ifndef SEMICRF_NFARW
#define SEMICRF_NFARW 2             // far waves per spine workgroup that exist (a launch uses 1 or 2: the next two)
#endif
#ifndef SEMICRF_NFARW2_MAXB
#define SEMICRF_NFARW2_MAXB 192     // forward / decode launches of at most this many chains ...
#endif
#ifndef SEMICRF_NFARW2_MINT
#define SEMICRF_NFARW2_MINT 1024    // ... and at least this many frames use two far waves per spine
#endif

// ---- panels --------------------------------------------------------------------------------------------------------------------
#ifndef SEMICRF_TPT
#define SEMICRF_TPT 12              // tiles per task: 12 and a last part of at least 4: 184-186 us vs 188-190 with 16 / 1 (T=1024, NBatch=352)
#endif
#ifndef SEMICRF_LEADT
#define SEMICRF_LEADT 4             // least length of a block's last part (tiles)
#endif
#ifndef SEMICRF_PNS
#define SEMICRF_PNS 3               // LDS stages per panel wave (tiles fetched ahead)
#endif
#ifndef SEMICRF_PW_MAX
#define SEMICRF_PW_MAX 5            // panel waves per workgroup (LDS: PW_MAX * PNS * 10 KB = 150 KB; four of them run unless the sweep is throughput-bound)
#endif
#ifndef SEMICRF_STAGGER
#define SEMICRF_STAGGER 32          // s_sleep units (64 cycles) per block of distance before a panel wave starts on its known first task
#endif
#ifndef SEMICRF_CELL_AUX
#define SEMICRF_CELL_AUX 2          // cache policy of the cell stream where it is non-temporal (2 = nt: every cell is read once)
#endif
#ifndef SEMICRF_NT_MIN_MB
#define SEMICRF_NT_MIN_MB 240       // lower triangles of at least this many MB are streamed non-temporal (see cell_policy_nt)
#endif

// ---- gradient sweep ------------------------------------------------------------------------------------------------------------
#ifndef SEMICRF_GRAD_LAZY
#define SEMICRF_GRAD_LAZY 127       // s_sleep units between a gradient-sweep panel wave's polls for a tile that is not its task's newest
#endif
#ifndef SEMICRF_GRAD_HSTART
#define SEMICRF_GRAD_HSTART 12      // the spine workgroups' spare waves stream from this row block on
#endif
#ifndef SEMICRF_GRAD_AUX
#define SEMICRF_GRAD_AUX 2          // cache policy of the marginals' stores (2 = nt: the gradient is written once)
#endif
#ifndef SEMICRF_GRAD_NT_MIN_MB
#define SEMICRF_GRAD_NT_MIN_MB 0    // ... for lower triangles of at least this many MB (0: always non-temporal)
#endif

// ---- in-sweep band copy (copy_role) --------------------------------------------------------------------------------------------
#ifndef SEMICRF_BANDX
#define SEMICRF_BANDX 1            // 1: launches with few chains copy the band into spine-major order while they run (copy_role) and
#endif                              //    their loaders read whole 128-byte lines; 0: the loader always reads the score tensor itself
#ifndef SEMICRF_BANDX_MAXB
#define SEMICRF_BANDX_MAXB 192     // ... for at most this many chains per launch (the copy moves the band twice more: at 352 chains
#endif                              //    that is 1.5 TB/s each way in the head of the sweep, where the hand-offs want a quiet fabric)
#ifndef SEMICRF_BAND_LOAD_AUX
#define SEMICRF_BAND_LOAD_AUX 16   // ... cache policy of the loader's loads from the copy (16 = sc1: written by another CU in this launch)
#endif
#ifndef SEMICRF_BANDX_WGSTRIDE
#define SEMICRF_BANDX_WGSTRIDE 3   // ... in every n-th panel workgroup (every one: the copy's burst delays the first hand-offs)
#endif
#ifndef SEMICRF_BANDX_WAVES
#define SEMICRF_BANDX_WAVES 1      // ... copy waves per panel workgroup (1 / 2 / 4: 127 / 130 / 139 us at T=1024 x 88)
#endif
#ifndef SEMICRF_BANDX_K0
#define SEMICRF_BANDX_K0 8         // ... row blocks below this one are loaded from the score tensor (the copy has not started yet)
#endif
