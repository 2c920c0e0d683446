// scorer_bwd_gemm3.h -- the two products of the packed interval-score backward on the bf16 matrix instructions, three exact limbs
// per operand (opt-in).  Included by scorer_bwd_gemm.hip.
#pragma once
#include "scorer_bwd_gemm_common.h"
#include "bf16x3.h"
#include "scorer_tuning.h"

namespace semicrf {

// ---------------------------------------------------------------------------------------------
// The same two products on the bf16 matrix instructions, every operand as three exact bf16 limbs (bf16x3.h; opt-in:
// length_scaling | SEMICRF_LEN_BF16X3).  Six instructions of 8 passes replace eight fp32 instructions of 16 per 16
// contraction values: 2.67x less matrix time, fp32-grade results (not bit-identical to the exact-fp32 kernel above).
// ---------------------------------------------------------------------------------------------
// Same items, same output tile (128 x D, wave = 32 rows x D/2 columns), same epilogue.  What differs is the operand path.
// v_mfma_f32_32x32x16_bf16 wants EIGHT consecutive contraction values of one row (A) / one column (B) per lane, and one of the
// two operands of either product has the contraction index as its ROW index in memory (k[b][:] for dq; Gt[e][:] and q[e][:] for
// dk).  So nothing goes from memory to LDS directly: every lane fetches "units" of eight contraction values into registers two
// chunks ahead -- a unit along a memory row is two 16-byte loads, a unit across rows is eight 4-byte loads of one column
// (consecutive lanes on consecutive columns: 256-byte runs; the row is wave-uniform and sits in the scalar offset of a buffer
// load, so a unit costs no address arithmetic in the vector unit) -- splits each value once (~5.5 vector instructions) and stores
// the three limbs as 16-byte pieces in exactly the layout the matrix instruction reads: [limb][row][4 pieces of 8 values],
// pieces swizzled by row as in the forward's three-limb kernel (reads conflict-free; the column units' writes two-way).
// Two LDS stages of 3 x (8 KB + D x 64 bytes) (144 KB at D = 256).
//
// Schedule.  Timing ablations of the first version (every wave: barrier, multiply, split the next chunk, request; T=1024 x 352,
// both products): matrix instructions alone 0.51 ms, everything 1.32 -- the parts ADD, because a barrier per chunk keeps the two
// waves of a SIMD in the same phase.  So the waves are two GROUPS (0-3 and 4-7: one of each per SIMD) half a chunk apart: while
// one group multiplies chunk n, the other splits its share of chunk n+1 and requests chunk n+3, then they swap; two barriers
// per chunk.  A multiplying wave has the SIMD's matrix pipe to itself, so its operand reads are issued one group of six
// instructions ahead (two sets of operand registers), the order pinned by scheduling barriers.
// That form is gone from the source; what runs is the interleaved form below (multiply_fill): every wave
// multiplies the chunk in one stage and, between its own matrix instructions, splits the next chunk into the other stage (a third
// of a piece behind every instruction) and requests the one after it; one barrier per chunk.  1.53 -> 1.45 ms at T=1024 x 352 at
// the clock's plateau (same box: two groups 1.528, interleaved with the requests behind the chunk 1.549, whole pieces 1.493, this 1.453).
// What the kernel is bound by, measured: DESIGN.md section 3 ("The last schedule, and what bounds it") and profiles/r05_mfma_peak.txt.
constexpr int G3_NS = 2;
constexpr int NXCD_G3 = 8;        // workgroup b runs on XCD b % 8
// Measured and removed (the code is in git history): the two-group schedule's variant with a slab's limb products
// round-robin over the accumulators (within 2 % of six in a row per accumulator, which is what multiply_fill issues), raised wave priority around a chunk's matrix instructions (+-1 %), no vmcnt(0) behind an item's stores
// (the same: 1.434-1.439 / 1.439-1.443 ms -- the next wait for a register set drains the stores anyway), a whole piece behind
// every third matrix instruction instead of a third behind every one, thirds in FRONT of a chunk's first instruction (3 the same,
// 6 one per cent slower), the younger wave of a SIMD first for 24 instructions (0.8 % SLOWER at the clock's plateau), and the
// requests behind the chunk instead of between its instructions (6 % slower).
template <bool AT, int NW>
__global__ __launch_bounds__(512, 2) void score_bwd_gemm3_kernel(const float* __restrict__ Gt, int Tp,
                                                                 const float* __restrict__ other, long long ldo,
                                                                 float* __restrict__ out, long long ldout, int C, int T,
                                                                 float* __restrict__ rsum, long long ldrs)
{
    constexpr int D = 64 * NW;
    constexpr int APL = GM * 64;                       // bytes of one limb plane of the Gt part: 128 rows x 32 values x 2 bytes
    constexpr int BPL = D * 64;                        // ... of the k/q part: D rows (columns of k/q)
    constexpr int BOFF = 3 * APL;
    constexpr int STAGE = 3 * (APL + BPL);
    constexpr int WPP = D / 128 > 0 ? D / 128 : 1;     // waves per piece (8 rows) of the k/q part: 64 column pairs per wave
    extern __shared__ __attribute__((aligned(16))) char glds[];    // [G3_NS][STAGE]: Gt limbs h | m | l | k/q limbs h | m | l
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int l31 = lane & 31, half = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;           // this wave: rows 32*wm.., columns 32*NW*wn.. of the tile
    const int nm = (T + GM - 1) / GM;
    const long long nitems = (long long)nm * C;
    const int nkt = Tp / GK;
    const size_t slab = gt_chain_floats(Tp);

    // Item order.  An output tile re-reads its chain's k (q) rows, 1 MB per chain at T=1024, and with tiles dealt chain-fastest (the
    // fp32 kernel's order: 256 workgroups on 256 chains) nearly all of that comes from memory: 2.4 GB per product, which the fp32
    // kernel's 1.0 ms does not notice and this kernel's matrix time (0.26 ms) does.  Here a chain's tiles run side by side on ONE
    // XCD (its L2 serves the other seven readers of a row): workgroup b = (XCD b % 8, slot b / 8); XCD x owns the chains c = x mod 8
    // and walks the list [chain][position] with its slots; the tile behind a position rotates from round to round, mirrored in
    // every other round (tiles a and nm-1-a together are one chain's average), so that the slots stay within a round of each other
    // although their tiles differ 8 : 1 in length.  All tiles of a chain start at the same end of the contraction (dk walks it
    // backwards).  Few chains (or a grid that is no multiple of 8): the plain order.
    // (with few items per slot the rotation cannot even out the tile lengths: T=691 x 90 chains 0.30 -> 0.38 ms in this order)
    const bool xcd_order = (gridDim.x % NXCD_G3) == 0 && C >= 8 * NXCD_G3 && (long long)C * nm >= 4 * (long long)gridDim.x;
    const int nslots = gridDim.x / NXCD_G3, xcd = blockIdx.x % NXCD_G3;
    const int cpr = nslots / nm > 0 ? nslots / nm : 1;               // chains of an XCD per round
    // the workgroup's item number `round` (32-bit arithmetic throughout: nm * C items)
    auto item_of = [&](int round, int& c, int& mi, int& kbeg, int& nk) -> bool {
        unsigned ti;
        if (xcd_order) {
            const unsigned nch = (unsigned)(C - xcd + NXCD_G3 - 1) / NXCD_G3;       // chains of this XCD
            const unsigned u = blockIdx.x / NXCD_G3 + (unsigned)nslots * (unsigned)round;
            if (u >= nch * (unsigned)nm) return false;
            const unsigned lc = u / (unsigned)nm, pos = u % (unsigned)nm, rr = lc / (unsigned)cpr;
            const unsigned base = (pos + (rr >> 1)) % (unsigned)nm;
            ti = (rr & 1) ? nm - 1 - base : base;                    // 0 = the longest contraction range
            c = __builtin_amdgcn_readfirstlane((int)(lc * NXCD_G3 + xcd));  // (divisions run in the vector unit: back to scalar registers)
        } else {
            const unsigned n = blockIdx.x + gridDim.x * (unsigned)round;
            if (n >= (unsigned)nitems) return false;
            ti = n / (unsigned)C;                                    // longest first
            c = __builtin_amdgcn_readfirstlane((int)(n % (unsigned)C));
        }
        mi = __builtin_amdgcn_readfirstlane(AT ? (int)ti : nm - 1 - (int)ti);
        if (AT) {
            kbeg = mi * (GM / GK);                                   // chunks nkt-1 down to kbeg
            nk = nkt - kbeg;
        } else {
            kbeg = 0;
            nk = (mi + 1) * (GM / GK) < nkt ? (mi + 1) * (GM / GK) : nkt;
        }
        return true;
    };

    // ---- reading lanes: lane = (row, half); the instruction of slab sl takes piece 2*half + sl of the row ----------------
    unsigned rdA[2], rdB[2];
    {
        const int ra = 32 * wm + l31, rb = 32 * NW * wn + l31;          // (column block t: + 32 rows = + 2048 bytes, same swizzle)
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) {
            rdA[sl] = (unsigned)(ra * 64 + (((2 * half + sl) ^ ((ra >> 2) & 3)) * 16));
            rdB[sl] = (unsigned)(BOFF + rb * 64 + (((2 * half + sl) ^ ((rb >> 2) & 3)) * 16));
        }
    }
    // ---- staging lanes --------------------------------------------------------------------------------------------------
    // Gt: dq -- unit = (row tid / 4, piece tid % 4) along the row; dk -- unit = (row = b = tid % 128, piece tid / 128) across rows e
    const int aRow = AT ? (tid & 127) : (tid >> 2);
    const int aPiece = AT ? (wave >> 1) : (tid & 3);
    const unsigned wA = (unsigned)(aRow * 64 + ((aPiece ^ ((aRow >> 2) & 3)) * 16));
    // k/q: a lane takes TWO adjacent columns (8-byte loads: half the vector-memory instructions of 4-byte ones, and the issue of
    // those -- 24 per wave and chunk -- was 17 % of a wave's time) of the 8 rows of one piece: units (column 2 cp + j, piece), j = 0, 1;
    // the piece is wave-uniform.  D = 256: all 512 lanes; D = 128: waves 0-3; D = 64: their lanes 0-31 (the others fetch a valid
    // address again and store nothing)
    const int bPieceRaw = wave / WPP, bCpRaw = (wave % WPP) * 64 + lane;
    const bool bOn = D >= 256 || (bPieceRaw < 4 && bCpRaw < D / 2);
    const int bPiece = bPieceRaw < 4 ? bPieceRaw : 3, bCp = bCpRaw < D / 2 ? bCpRaw : D / 2 - 1;
    unsigned wB[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int d = 2 * bCp + j;
        wB[j] = (unsigned)(BOFF + d * 64 + ((bPiece ^ ((d >> 2) & 3)) * 16));
    }
    const unsigned bVoff = (unsigned)(bCp * 8);

    // ---- request side (identical in all waves) ---------------------------------------------------------------------------
    // (per item: the buffer descriptors of the chain's slabs and the block offset; per chunk the scalar unit computes 32-bit
    // offsets by increments -- the first version's 64-bit address arithmetic was ~500 scalar instructions per wave and chunk,
    // 4000 issue cycles of the CU's one scalar unit against 3072 matrix cycles)
    typedef int v4i __attribute__((ext_vector_type(4)));
    auto make_rsrc = [](const void* p, size_t bytes) -> v4i {
        const unsigned long long a = (unsigned long long)(uintptr_t)p;
        return (v4i){(int)(unsigned)a, (int)((a >> 32) & 0xffffu), (int)(unsigned)bytes, 0x00020000};
    };
    const unsigned ldo4 = (unsigned)(ldo * 4), somax = (unsigned)(T - 1) * ldo4;
    int nx_round = 0;
    int nx_c = 0, nx_mi = 0, nx_kbeg = 0, nx_nk = 0, nx_j = 0;
    bool nx_valid = item_of(nx_round, nx_c, nx_mi, nx_kbeg, nx_nk);
    if (!nx_valid) return;                             // uniform
    unsigned aVoff = AT ? (unsigned)((tid & 127) * 4) : 0u;
    v4i nx_ra, nx_rb;
    unsigned nx_aoff = 0;                              // dq: byte offset of the item's 128-row block of Gt
    auto set_item_offsets = [&]() {
        nx_ra = make_rsrc(Gt + (size_t)nx_c * slab, slab * 4);
        nx_rb = make_rsrc(other + (size_t)nx_c * T * ldo, ((size_t)(T - 1) * ldo + D) * 4);
        if (!AT) {
            const int rows = Tp - nx_mi * GM < GM ? Tp - nx_mi * GM : GM;      // rows of the block that exist (the others are not stored)
            const int R = aRow < rows ? aRow : rows - 1;
            aVoff = (unsigned)((R * gt_row_len(nx_mi, Tp) + aPiece * 8) * 4);
            nx_aoff = (unsigned)(gt_block_off(nx_mi) * 4);
        }
    };
    set_item_offsets();

    // Requests and their waits are written out (asm): the compiler's own bookkeeping of loads in flight turned the wait for
    // the OLDER register set into a wait for everything in every other step (vmcnt 17 -> 0 where 35 -> 18 was meant, with and
    // without the epilogue's stores in the loop), i.e. a stall of one memory latency per chunk -- timing ablations: without the
    // requests 1.35 ms, without the split 1.34, without both 1.33, complete 1.99.  Here a set's NLD loads are issued back to
    // back, nothing else is in flight except the other set's NLD (the epilogue drains its stores), and the wait in front of
    // a set's split is vmcnt(NLD).  The loaded registers are tied to that wait ("+v"): no use can move above it; the loads are
    // UNCONDITIONAL (past the last chunk the last one is fetched again and never used) so that the count is always the same.
    constexpr int NLD = (AT ? 8 : 2) + 8;
    struct Regs { v4f alo, ahi; float a[8]; f32x2 b[8]; };
    struct Meta { bool valid, last; int c, mi; };
    // A request for one chunk = prepare (the chunk's scalar offsets, and the walk over the items moves on) + issue (the loads; the
    // interleaved schedule issues them between its matrix instructions, the B loads and the A loads at different places).
    struct Pend { v4i ra, rb; unsigned av, sa, krl4, sr; };
    auto prepare = [&](Meta& m, Pend& q) __attribute__((always_inline)) {
        m.valid = nx_valid;
        const unsigned k0 = (unsigned)(AT ? nkt - 1 - nx_j : nx_kbeg + nx_j) * GK;
        q.ra = nx_ra; q.rb = nx_rb; q.av = aVoff; q.krl4 = 0;
        if (!AT) {
            q.sa = nx_aoff + k0 * 4;
        } else {
            // the chunk's 32 rows (e) lie in one 128-row block; columns past the block's row length (a last block that is not
            // 128 wide) read the next row or the workspace's slack: they only reach output rows >= T, which are not written
            const unsigned kblk = k0 / GM;
            q.krl4 = (unsigned)gt_row_len((int)kblk, Tp) * 4;
            q.sa = (unsigned)GM * GM * 4 * (kblk * (kblk + 1) / 2) + (k0 - kblk * GM + 8 * aPiece) * q.krl4 + (unsigned)nx_mi * (GM * 4);
        }
        q.sr = (k0 + 8 * bPiece) * ldo4;                         // rows past T meet Gt == 0: any finite value will do (the last row's)
        m.last = nx_j + 1 == nx_nk;
        m.c = nx_c;
        m.mi = nx_mi;
        if (nx_valid && ++nx_j == nx_nk) {
            int c2, mi2, kbeg2, nk2;
            if (item_of(nx_round + 1, c2, mi2, kbeg2, nk2)) {
                ++nx_round;
                nx_c = c2; nx_mi = mi2; nx_kbeg = kbeg2; nx_nk = nk2; nx_j = 0;
                set_item_offsets();
            } else {
                nx_valid = false;
                nx_j = nx_nk - 1;
            }
        }
    };
    auto issue_a = [&](Regs& g, const Pend& q, int i0, int n) __attribute__((always_inline)) {     // AT: loads i0 .. i0 + n - 1 of 8; else both
        if (!AT) {
            asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(g.alo) : "v"(q.av), "s"(q.ra), "s"(q.sa));
            asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen offset:16" : "=v"(g.ahi) : "v"(q.av), "s"(q.ra), "s"(q.sa));
        } else {
#pragma unroll
            for (int i = i0; i < i0 + n; ++i) {
                const unsigned so = q.sa + (unsigned)i * q.krl4;
                asm volatile("buffer_load_dword %0, %1, %2, %3 offen" : "=v"(g.a[i]) : "v"(q.av), "s"(q.ra), "s"(so));
            }
        }
    };
    auto issue_b = [&](Regs& g, const Pend& q, int i0, int n) __attribute__((always_inline)) {
#pragma unroll
        for (int i = i0; i < i0 + n; ++i) {
            const unsigned sr = q.sr + (unsigned)i * ldo4;
            const unsigned so = sr < somax ? sr : somax;
            asm volatile("buffer_load_dwordx2 %0, %1, %2, %3 offen" : "=v"(g.b[i]) : "v"(bVoff), "s"(q.rb), "s"(so));
        }
    };
    auto fetch = [&](Regs& g, Meta& m) __attribute__((always_inline)) {
        Pend q;
        prepare(m, q);
        issue_a(g, q, 0, 8);
        issue_b(g, q, 0, 8);
    };
    // the set's loads have landed (the other set's NLD younger ones may be in flight)
    auto landed = [&](Regs& g) {
        asm volatile("s_waitcnt vmcnt(%0)" :: "n"(NLD));
        if (!AT) {
            asm volatile("" : "+v"(g.alo), "+v"(g.ahi));
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) asm volatile("" : "+v"(g.a[i]));
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) asm volatile("" : "+v"(g.b[i]));
    };
    float rs = 0.0f;                                    // !AT && rsum: this lane's part of its row's sum
    const bool want_rs = !AT && rsum != nullptr;
    auto convert = [&](Regs& g, const Meta& m, int stage) {
        char* base = glds + stage * STAGE;
        v4f alo, ahi;
        if (AT) { alo = (v4f){g.a[0], g.a[1], g.a[2], g.a[3]}; ahi = (v4f){g.a[4], g.a[5], g.a[6], g.a[7]}; }
        else { alo = g.alo; ahi = g.ahi; }
        {
            const Limbs3 L = split8(alo, ahi);
            *(bf16x8*)(base + wA) = L.h;
            *(bf16x8*)(base + APL + wA) = L.m;
            *(bf16x8*)(base + 2 * APL + wA) = L.l;
        }
        if (!AT && want_rs && m.valid) {
            rs = add1(rs, add1(add1(add1(alo.x, alo.y), add1(alo.z, alo.w)), add1(add1(ahi.x, ahi.y), add1(ahi.z, ahi.w))));
            if (m.last) {
                float tot = rs + __shfl_xor(rs, 1);
                tot += __shfl_xor(tot, 2);
                const int mrow = m.mi * GM + aRow;
                if ((tid & 3) == 0 && mrow < T) rsum[((size_t)m.c * T + mrow) * ldrs] = tot;
                rs = 0.0f;
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const Limbs3 L = split8((v4f){g.b[0][j], g.b[1][j], g.b[2][j], g.b[3][j]}, (v4f){g.b[4][j], g.b[5][j], g.b[6][j], g.b[7][j]});
            if (D >= 256 || bOn) {
                *(bf16x8*)(base + wB[j]) = L.h;
                *(bf16x8*)(base + BPL + wB[j]) = L.m;
                *(bf16x8*)(base + 2 * BPL + wB[j]) = L.l;
            }
        }
    };

    f32x16 acc[NW];
#pragma unroll
    for (int t = 0; t < NW; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    // The SAME wave splits the next chunk between its own matrix instructions -- one
    // piece (a pair of values through the three-limb split, or a unit's three limb stores) behind every third instruction, the order
    // pinned by scheduling barriers.  Cycle stamps and priority experiments of the two-group schedule said why: a SIMD issues to its
    // oldest wave first, so whichever group is older runs at full speed and the other one starves (multiply 1960 cycles per chunk for
    // the waves 0-3, 2950 for 4-7; with raised priority for 4-7 it is the other way round) -- the split next to ANOTHER wave's matrix
    // instructions does not overlap, the split between a wave's OWN matrix instructions does (a filler per instruction is nearly free).
    auto mma1 = [&](const Limbs3& A, const Limbs3& B, f32x16& ac, int pz) __attribute__((always_inline)) {
        switch (pz) {
        case 0: ac = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A.h, B.l, ac, 0, 0, 0); break;
        case 1: ac = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A.l, B.h, ac, 0, 0, 0); break;
        case 2: ac = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A.m, B.m, ac, 0, 0, 0); break;
        case 3: ac = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A.h, B.m, ac, 0, 0, 0); break;
        case 4: ac = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A.m, B.h, ac, 0, 0, 0); break;
        default: ac = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A.h, B.h, ac, 0, 0, 0); break;
        }
    };
    // NW = 4: the chunk after next is requested from inside, too -- the k/q columns first through the split (pieces
    // 0-9), their loads two at a time behind the instructions 30, 33, 36, 39, the Gt unit last (pieces 10-14) and its loads behind
    // 45 and 46: the address path works while the matrix pipe does, instead of ~550 cycles per wave behind the chunk.
    constexpr bool FL = NW == 4;
    auto multiply_fill = [&](int stage, Regs& g, Meta& mref, int wstage) __attribute__((always_inline)) {
        const char* base = glds + stage * STAGE;
        char* wbase = glds + wstage * STAGE;
        const Meta m = mref;
        Pend q;
        if (FL) prepare(mref, q);
        // the values to split: unit 0 = the Gt unit, units 1, 2 = the two k/q columns of the lane's pair
        v4f alo, ahi;
        if (AT) { alo = (v4f){g.a[0], g.a[1], g.a[2], g.a[3]}; ahi = (v4f){g.a[4], g.a[5], g.a[6], g.a[7]}; }
        else { alo = g.alo; ahi = g.ahi; }
        unsigned ph[4], pm[4], pl[4];
        auto pairv = [&](int u, int pr, float& x, float& y) __attribute__((always_inline)) {
            if (u == 0) {
                const v4f v = pr < 2 ? alo : ahi;
                x = (pr & 1) ? v.z : v.x; y = (pr & 1) ? v.w : v.y;
            } else {
                x = g.b[2 * pr][u - 1]; y = g.b[2 * pr + 1][u - 1];
            }
        };
        auto piece = [&](int k) __attribute__((always_inline)) {             // k = 0 .. 14: (unit, step k % 5)
            const int u = FL ? (k < 10 ? 1 + k / 5 : 0) : k / 5, st = k % 5;
            if (st < 4) {
                float x, y;
                pairv(u, st, x, y);
                split_pair(x, y, ph[st], pm[st], pl[st]);
            } else {
                const unsigned wo = u == 0 ? wA : wB[u - 1];
                const int pitch = u == 0 ? APL : BPL;
                if (u == 0 || D >= 256 || bOn) {
                    *(u32x4*)(wbase + wo) = (u32x4){ph[0], ph[1], ph[2], ph[3]};
                    *(u32x4*)(wbase + pitch + wo) = (u32x4){pm[0], pm[1], pm[2], pm[3]};
                    *(u32x4*)(wbase + 2 * pitch + wo) = (u32x4){pl[0], pl[1], pl[2], pl[3]};
                }
                if (u == 0 && !AT && want_rs && m.valid) {
                    rs = add1(rs, add1(add1(add1(alo.x, alo.y), add1(alo.z, alo.w)), add1(add1(ahi.x, ahi.y), add1(ahi.z, ahi.w))));
                    if (m.last) {
                        float tot = rs + __shfl_xor(rs, 1);
                        tot += __shfl_xor(tot, 2);
                        const int mrow = m.mi * GM + aRow;
                        if ((tid & 3) == 0 && mrow < T) rsum[((size_t)m.c * T + mrow) * ldrs] = tot;
                        rs = 0.0f;
                    }
                }
            }
        };
        // the same work in thirds (NW = 4): a split level (convert, widen, subtract: 5 instructions) or one limb plane's store
        // behind EVERY matrix instruction -- a whole piece is 13 dependent-ish vector instructions, longer than the instruction in
        // front of it runs, and the wave's next matrix instruction waits behind them
        f32x2 srem = {0.0f, 0.0f};
        float rsa = 0.0f;
        auto subpiece = [&](int k3) __attribute__((always_inline)) {         // k3 = 0 .. 44: (piece k3 / 3, part k3 % 3)
            const int k = k3 / 3, part = k3 % 3;
            const int u = FL ? (k < 10 ? 1 + k / 5 : 0) : k / 5, st = k % 5;
            if (st < 4) {
                if (part == 0) {
                    float x, y;
                    pairv(u, st, x, y);
                    const unsigned hu = cvt_pk_bf16(x, y);
                    const f32x2 xv = {x, y}, hf = {__builtin_bit_cast(float, hu << 16), __builtin_bit_cast(float, hu & 0xffff0000u)};
                    ph[st] = hu;
                    srem = sub2(xv, hf);
                } else if (part == 1) {
                    const unsigned mu = cvt_pk_bf16(srem.x, srem.y);
                    const f32x2 mf = {__builtin_bit_cast(float, mu << 16), __builtin_bit_cast(float, mu & 0xffff0000u)};
                    pm[st] = mu;
                    srem = sub2(srem, mf);
                } else {
                    pl[st] = cvt_pk_bf16(srem.x, srem.y);
                }
            } else {
                const unsigned wo = u == 0 ? wA : wB[u - 1];
                const int pitch = u == 0 ? APL : BPL;
                if (u == 0 || D >= 256 || bOn) {
                    if (part == 0) *(u32x4*)(wbase + wo) = (u32x4){ph[0], ph[1], ph[2], ph[3]};
                    else if (part == 1) *(u32x4*)(wbase + pitch + wo) = (u32x4){pm[0], pm[1], pm[2], pm[3]};
                    else *(u32x4*)(wbase + 2 * pitch + wo) = (u32x4){pl[0], pl[1], pl[2], pl[3]};
                }
                if (u == 0 && !AT && want_rs && m.valid) {
                    if (part == 0) rsa = add1(add1(alo.x, alo.y), add1(alo.z, alo.w));              // (the same order as piece())
                    else if (part == 1) rs = add1(rs, add1(rsa, add1(add1(ahi.x, ahi.y), add1(ahi.z, ahi.w))));
                    else if (m.last) {
                        float tot = rs + __shfl_xor(rs, 1);
                        tot += __shfl_xor(tot, 2);
                        const int mrow = m.mi * GM + aRow;
                        if ((tid & 3) == 0 && mrow < T) rsum[((size_t)m.c * T + mrow) * ldrs] = tot;
                        rs = 0.0f;
                    }
                }
            }
        };
        Limbs3 A, B[2];
        auto ldA = [&](Limbs3& L, int sl) __attribute__((always_inline)) {
            L.h = *(const bf16x8*)(base + rdA[sl]);
            L.m = *(const bf16x8*)(base + APL + rdA[sl]);
            L.l = *(const bf16x8*)(base + 2 * APL + rdA[sl]);
        };
        auto ldB = [&](Limbs3& L, int sl, int t) __attribute__((always_inline)) {
            L.h = *(const bf16x8*)(base + rdB[sl] + t * 2048);
            L.m = *(const bf16x8*)(base + BPL + rdB[sl] + t * 2048);
            L.l = *(const bf16x8*)(base + 2 * BPL + rdB[sl] + t * 2048);
        };
        ldA(A, 0);
        ldB(B[0], 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        static_for<0, 2 * NW>([&](auto ic) __attribute__((always_inline)) {
            constexpr int i = decltype(ic)::value;
            constexpr int t = i % NW;
            if constexpr (i + 1 < 2 * NW && (i + 1) % NW != 0 && !(SEMICRF_G3_ABL & 2)) ldB(B[(i + 1) & 1], (i + 1) / NW, (i + 1) % NW);
            __builtin_amdgcn_sched_barrier(0);
            static_for<0, 6>([&](auto pc) __attribute__((always_inline)) {
                constexpr int pz = decltype(pc)::value;
                constexpr int n = 6 * i + pz;                              // 0 .. 12 NW - 1
                mma1(A, B[(SEMICRF_G3_ABL & 2) ? 0 : (i & 1)], acc[t], pz);
                __builtin_amdgcn_sched_barrier(0);
                constexpr int every = (12 * NW) / 15 > 0 ? (12 * NW) / 15 : 1;       // NW = 4: a piece behind every third instruction
                constexpr bool FINE = NW == 4;
                if constexpr (FINE && n < 45 && !(SEMICRF_G3_ABL & 1)) {
                    subpiece(n);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (!FINE && n % every == every - 1 && n / every < 15 && !(SEMICRF_G3_ABL & 1)) {
                    piece(n / every);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (FL && n >= 30 && n <= 39 && n % 3 == 0 && !(SEMICRF_G3_ABL & 4)) {
                    issue_b(g, q, 2 * ((n - 30) / 3), 2);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (FL && (n == 45 || (AT && n == 46)) && !(SEMICRF_G3_ABL & 4)) {
                    issue_a(g, q, 4 * (n - 45), 4);
                    __builtin_amdgcn_sched_barrier(0);
                }
            });
            if constexpr (i + 1 < 2 * NW && (i + 1) % NW == 0 && !(SEMICRF_G3_ABL & 2)) {
                ldA(A, (i + 1) / NW);
                ldB(B[(i + 1) & 1], (i + 1) / NW, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        });
        // (NW < 4: fewer instructions than pieces -- the rest of the split behind the last one)
        static_for<0, 15>([&](auto kc) __attribute__((always_inline)) {
            constexpr int k = decltype(kc)::value;
            constexpr int every = (12 * NW) / 15 > 0 ? (12 * NW) / 15 : 1;
            if constexpr (k >= (12 * NW) / every) piece(k);
        });
    };

    Regs gX, gY;
    Meta mX = {false, false, 0, 0}, mY = {false, false, 0, 0};
    auto sync = [&]() {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // my limb stores are in the LDS ...
        __builtin_amdgcn_s_barrier();                            // ... and so are everybody's; everybody is done reading the other stage
        asm volatile("" ::: "memory");
    };
    // prologue: chunk 0 is split by everybody in front of the first barrier.  X is the register set split in the steps with P = 0, Y
    // with P = 1.
    fetch(gY, mY);
    fetch(gX, mX);
    landed(gY);
    convert(gY, mY, 0);
    fetch(gY, mY);

    int cur_round = 0;
    int c = 0, mi = 0, kbeg = 0, nk = 0, j = 0;
    (void)item_of(cur_round, c, mi, kbeg, nk);
    // ---- the item's 128 x D block (C/D layout: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)); rows >= T are
    //      dropped by the buffer's range check (the row sits in the per-lane offset): no branches.  Then ONE wait for everything
    //      in flight: stores and loads complete out of order with respect to each other, so with a store pending the compiler
    //      turns every later wait for a load into vmcnt(0) -- on every path through that wait, i.e. in every chunk (the first
    //      version: 17 -> 0 where 35 -> 18 was meant).  Draining here, once per item, keeps the chunks' waits exact. ----
    auto finish = [&]() -> bool {
        if (++j < nk) return true;
        const auto ro = __builtin_amdgcn_make_buffer_rsrc((void*)(out + (size_t)c * T * ldout), 0, (int)((size_t)T * ldout * 4), 0x00020000);
        const unsigned v0 = (unsigned)(((size_t)(mi * GM + 32 * wm + 4 * half) * ldout + 32 * NW * wn + l31) * 4);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned vr = v0 + (unsigned)((size_t)((r & 3) + 8 * (r >> 2)) * ldout * 4);
#pragma unroll
            for (int t = 0; t < NW; ++t) {
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc[t][r]), ro, vr, t * 128, 0);     // (not __builtin_bit_cast of a vector element: bf16x3.h)
                acc[t][r] = 0.0f;
            }
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);                      // vmcnt(0)
        j = 0;
        return item_of(++cur_round, c, mi, kbeg, nk);
    };
#if SEMICRF_G3_PROBE
    unsigned long long pc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, pt = __builtin_readcyclecounter();
    const unsigned long long rt0 = __builtin_amdgcn_s_memrealtime();          // 100 MHz
#if SEMICRF_G3_PROBE == 2         // (2: the kernel's own clock -- one stamp at each end of a wave's life, nothing in the loop)
#define G3_STAMP(i) do { } while (0)
#else
#define G3_STAMP(i) do { const unsigned long long now_ = __builtin_readcyclecounter(); pc[i] += now_ - pt; pt = now_; } while (0)
#endif
#else
#define G3_STAMP(i) do { } while (0)
#endif
    // one chunk (ONE barrier): its limbs are in stage P; every wave multiplies it and splits the next chunk into the other stage between
    // its matrix instructions
    auto step = [&](auto PC, Regs& gn, Meta& mn) __attribute__((always_inline)) -> bool {
        constexpr int P = decltype(PC)::value;
        sync();
        G3_STAMP(2);
        landed(gn);
        G3_STAMP(3);
        multiply_fill(P, gn, mn, P ^ 1);
        G3_STAMP(0);
        const bool more = finish();
        G3_STAMP(1);
        if (!FL) fetch(gn, mn);
        G3_STAMP(5);
        return more;
    };
    while (true) {
        if (!step(std::integral_constant<int, 0>{}, gX, mX)) break;
        if (!step(std::integral_constant<int, 1>{}, gY, mY)) break;
    }
#if SEMICRF_G3_PROBE
    if (SEMICRF_G3_PROBE == 2) pc[0] = __builtin_readcyclecounter() - pt;
    pc[7] = __builtin_amdgcn_s_memrealtime() - rt0;
    __syncthreads();
    if (lane == 0 && rsum)        // (behind the C x T row sums: the probe script allocates 16 K floats more)
        for (int i = 0; i < 8; ++i) rsum[(size_t)C * T * ldrs + (size_t)(blockIdx.x * 8 + wave) * 8 + i] = (float)pc[i];
#endif
#undef G3_STAMP
}

template <bool AT, int NW>
static void launch_gemm3(const float* Gt, int Tp, const float* other, long long ldo, float* out, long long ldout, int C,
                        int T, hipStream_t stream, float* rsum = nullptr, long long ldrs = 1)
{
    const size_t lds = (size_t)G3_NS * 3 * (GM * 64 + 64 * NW * 64);
    static PerDeviceOnce attr_once;
    if (attr_once.first()) {
        (void)hipFuncSetAttribute((const void*)score_bwd_gemm3_kernel<AT, NW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    }
    const int grid = persistent_grid(device_ncu(), 1, (long long)((T + GM - 1) / GM) * C);      // one workgroup per CU, at most one per item
    hipLaunchKernelGGL((score_bwd_gemm3_kernel<AT, NW>), dim3(grid), dim3(512), lds, stream, Gt, Tp, other, ldo, out, ldout, C, T,
                       AT ? nullptr : rsum, ldrs);
}

}  // namespace semicrf
