// fp32-equivalent GEMMs on the 16-bit matrix pipe (SURVEY.md 7 lists the route).
//
// gfx950 has no tf32 / xf32 MFMA: an exact-f32 product costs v_mfma_f32_32x32x2_f32 = 1/16 of the bf16 rate.  Split every
// f32 operand into NPL bf16 pieces (round-to-nearest-even, the residual is exact in f32):
//     a = a0 + a1 + a2 + e,   |a1| <= 2^-9 |a|,  |a2| <= 2^-18 |a|,  |e| <= 2^-27 |a|          (8 + 8 + 8 significand bits)
// and a product of two pieces (8 x 8 bits) is exact in the MFMA's f32 accumulator, so
//     NPL = 3:  a b ~= a0 b0 + (a0 b1 + a1 b0) + (a0 b2 + a1 b1 + a2 b0)      6 MFMAs, dropped terms <= 3 * 2^-27 |a b|
//     NPL = 2:  a b ~= a0 b0 + (a0 b1 + a1 b0)                                3 MFMAs, dropped terms <= 3 * 2^-18 |a b|
// i.e. NPL = 3 carries the operands' full 24 bits (the dropped part is below f32's own 2^-24 rounding of each
// accumulation) at 6/16 of the f32-MFMA cycles; NPL = 2 is a 16-bit-significand mode at 3/16.  Accumulation is f32 in both.
// This is NOT the bit-exact fmaf chain of the native kernels (different rounding points).  NPL = 2 (gemm_split2i_kernel) is an opt-in engine mode
// (IRSDE_FLAG_SPLIT_BF16X2 / _F16X2) with its own measured error table (profiles/r03_split_gemm_*.txt).  NPL = 3 (gemm_split3i_kernel) is fp32-equivalent
// and the exact-fp32 engine's default for its deep component GEMMs (profiles/split3.md; IRSDE_FLAG_NO_SPLIT3 restores the f32 MFMA kernels bit for bit).
//
// Where: the component GEMMs of the three-launch Winograd layers, M_z[t][n] = sum_c V_z[t][c] U_z[n][c] (reference call site:
// Block.proj, module_util.py:108-122).  wino.hip writes V already split (2 NPL bytes per element instead of 4) in the kernel's interleaved
// layout, U is split once at weight load, so the kernels below are pure 16-bit GEMMs over NPL + NPL operand pieces; the plane-major
// split_planes_kernel makes the pair copies of the fused kernels' weights (engine.h).
#include "common.h"
#include <algorithm>
#include <atomic>
#include <type_traits>

namespace irsde {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned uintx4 __attribute__((ext_vector_type(4)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int SG_BK = 32;            // k per K-step and plane

// ---------------------------------------------------------------------------------------------------------------
// The engine's kernel: two planes, pair-interleaved operands, LDS-DMA, 256 x 256 tiles.  Its predecessor (v2, removed: plane-major
// operands, register-staged ds_write_b128, same tiles; numbers in profiles/r03_split_gemm_notes.md) showed with ablation twins that
// without its global loads the K loop takes 69 % of the time and without MFMAs 72 %: the 64 wave-loads of a K-step (1 KB each, but
// 16 separate 64-byte row segments) cost as much as the 96 MFMAs they feed, and the 64 ds_write_b128 (13 cycles each) and their
// VGPR staging come on top.  Here:
//   * operand layout [row][k / 32][plane][32 k]: the hi and lo pieces of a row's 32-k block are ONE 128-byte line, so a wave-load
//     of 1 KB covers 8 rows x 128 B = 8 full lines instead of 16 half lines (wino_input / split_planes write this layout);
//   * global_load_lds_dwordx4: global -> LDS without VGPRs or ds_write; the LDS image of a stage is lane-linear (1 KB per
//     wave-load = 8 rows), the XOR swizzle of the 16-byte pieces (by (row >> 1) & 7: conflict-free ds_read_b128 lane groups on
//     128-byte rows) is applied to the per-lane SOURCE address and to the fragment reads (cdna_hip_programming.md rule 21);
//   * the loads of K-step t+1 are issued right after the barrier that ends step t-1 and have the whole MFMA phase of step t to
//     land; __syncthreads() (vmcnt(0) + s_barrier) ends the step.
// Block tile 256 x 256, 8 waves of 128 x 64, K-step 32, two LDS stages of 64 KB.
// ---------------------------------------------------------------------------------------------------------------
#define IRSDE_GLDS16(GPTR, LPTR) \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(GPTR), (__attribute__((address_space(3))) void*)(LPTR), 16, 0, 0)

// ABL: measurement twins (irsde_bench_conv 473 / 475 / 476): 1 = no global loads in the K loop, 3 = no MFMAs, 4 = no output stores;
// 5 = output stores with the non-temporal hint (IRSDE_SPLIT_NT=1 under IRSDE_TUNING=1 makes it the fp16 instance).  Measured, not used:
// the GEMMs +-1 %, but wino_output, which reads M right after, 5 - 10 % slower (M no longer waits in the L2 / Infinity Cache): 28.66 vs 28.72 ms
// F16: the two pieces are IEEE binary16 (11 significand bits each: hi + lo carry 22+ of f32's 24 bits, products exact in f32) on
// v_mfma_f32_32x32x16_f16 — fp32-equivalent per product at the same three MFMAs; the writers scale the operands by powers of two
// into fp16's range and g.out_scale undoes it here.
template <int ABL = 0, bool F16 = false>
__global__ __launch_bounds__(512, 2) void gemm_split2i_kernel(const SplitGemmArgs g) {
    using frag_t = typename std::conditional<F16, f16x8, bf16x8>::type;
    constexpr int TM = 4, TN = 2, WN = 4, BM = 256, BN = 256;
    constexpr int A_STAGE = BM * 128, STAGE = (BM + BN) * 128;   // bytes
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, h = lane >> 5;
    // XCD-aware work assignment (workgroup id w runs on XCD w % 8): a unit = (component, row tile) with all its column tiles;
    // XCD x owns the contiguous unit range [x U / 8, (x + 1) U / 8).  An A row tile is then read through ONE L2 (its column
    // tiles run side by side on that XCD and walk K in step), a component's B through at most two; with the plain
    // (tile, component) grid every A tile crossed two L2s and every B tile four, and the kernel sat on the HBM floor of
    // that traffic (v3 without MFMAs = 0.19 of its 0.25 ms, profiles/r03_split_gemm_notes.md).
    const int mtiles = (g.M + BM - 1) / BM;
    const int units = mtiles * g.n_inner;          // (n_inner carries the component count here)
    const int xcd = blockIdx.x & 7, jx = blockIdx.x >> 3;
    const int ulo = (int)((long long)xcd * units / 8), uhi = (int)((long long)(xcd + 1) * units / 8);
    const int unit = ulo + jx / g.nblk_n;
    if (unit >= uhi) return;
    const int nblk = jx % g.nblk_n;
    const int plane0 = unit / mtiles, mblk = unit - plane0 * mtiles;
    const int m0 = mblk * BM, n0 = nblk * BN;
    const int nk = g.K / SG_BK;
    const int steps = nk;
    const unsigned rowb = (unsigned)nk * 128u;   // bytes per operand row: K / 32 blocks of (hi 64 B | lo 64 B)

    // staging: wave-load (pass ps) = LDS chunk c = ps * 8 + wave = rows 8c .. 8c+7 of the A (B) tile; lane = (row 8c + lane / 8, slot lane % 8)
    // fetches the row's piece slot ^ ((row >> 1) & 7)
    unsigned a_voff[4], b_voff[4];
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
        const int row = (ps * 8 + wave) * 8 + (lane >> 3);
        const unsigned pc = (unsigned)((lane & 7) ^ ((row >> 1) & 7)) * 16u;
        int m = m0 + row;
        m = m < g.M ? m : g.M - 1;
        a_voff[ps] = (unsigned)m * rowb + pc;
        int n = n0 + row;
        n = n < g.N ? n : g.N - 1;
        b_voff[ps] = (unsigned)n * rowb + pc;
    }
    const char* abase = reinterpret_cast<const char*>(g.a);
    const char* bbase = reinterpret_cast<const char*>(g.b);
    const long long pA2 = g.pA * 4, pB2 = g.pB * 4;   // bytes between components: 2 planes x 2 bytes per element
    int kb = 0;
    const char* acomp = abase + (long long)plane0 * pA2;
    const char* bcomp = bbase + (long long)plane0 * pB2;
    auto issue_loads = [&](int buf) {
        char* la = lds + buf * STAGE + wave * 1024;
        const char* ga = acomp + kb * 128;
        const char* gb = bcomp + kb * 128;
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) IRSDE_GLDS16(ga + a_voff[ps], la + ps * 8192);
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) IRSDE_GLDS16(gb + b_voff[ps], la + A_STAGE + ps * 8192);
    };

    auto issue_loads_part = [&](int buf, int part) {   // the 8 loads of a stage in three groups: A 0-2 | A 3, B 0-1 | B 2-3
        char* la = lds + buf * STAGE + wave * 1024;
        const char* ga = acomp + kb * 128;
        const char* gb = bcomp + kb * 128;
        if (part == 0) {
            IRSDE_GLDS16(ga + a_voff[0], la);
            IRSDE_GLDS16(ga + a_voff[1], la + 8192);
            IRSDE_GLDS16(ga + a_voff[2], la + 2 * 8192);
        } else if (part == 1) {
            IRSDE_GLDS16(ga + a_voff[3], la + 3 * 8192);
            IRSDE_GLDS16(gb + b_voff[0], la + A_STAGE);
            IRSDE_GLDS16(gb + b_voff[1], la + A_STAGE + 8192);
        } else {
            IRSDE_GLDS16(gb + b_voff[2], la + A_STAGE + 2 * 8192);
            IRSDE_GLDS16(gb + b_voff[3], la + A_STAGE + 3 * 8192);
        }
    };

    floatx16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    issue_loads(0);
    __syncthreads();

    const int wm_s = wm, wn_s = wn;
    unsigned o_voff[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) o_voff[r] = (unsigned)(((r & 3) + 8 * (r >> 2) + 4 * h) * g.ldc + l31) * 4u;
    auto flush = [&](int fi) {
        const int rowb_ = m0 + wm_s * TM * 32, colb = n0 + wn_s * TN * 32;
        float* ob = g.out + (long long)(plane0 + fi) * g.pO + (long long)rowb_ * g.ldc;
        const int rows = g.M - rowb_;
        const unsigned nrec = rows <= 0 ? 0u : (unsigned)(rows < TM * 32 ? rows : TM * 32) * (unsigned)g.ldc * 4u;
        const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(ob, 0, nrec, 0x00020000);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int colu = colb + j * 32;
                if (colu + l31 < g.N && (ABL != 4 || acc[i][j][0] == 1.2345e30f)) {
                    const int soff = (i * 32 * g.ldc + colu) * 4;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float v = F16 ? acc[i][j][r] * g.out_scale : acc[i][j][r];   // (exact: a power of two)
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ro, (int)o_voff[r], soff, ABL == 5 ? 2 : 0);
                    }
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
            }
    };
    // fragment offsets inside a 128-byte row: piece = plane * 4 + sb * 2 + h, swizzled by (l31 >> 1) & 7 (tile bases are multiples of 32 rows)
    const int swz = (l31 >> 1) & 7;
    int fr_off[2][2];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int sb = 0; sb < 2; ++sb) fr_off[p][sb] = l31 * 128 + (((p * 4 + sb * 2 + h) ^ swz) * 16);
    for (int st = 0; st < steps; ++st) {
        const int buf = st & 1;
        const bool more = st + 1 < steps;
        if (more) ++kb;   // (stage buf^1 was last read in step st-1: every wave is past that step's barrier when the loads below are issued)
        const char* a = lds + buf * STAGE + wm * TM * 32 * 128;
        const char* b = lds + buf * STAGE + A_STAGE + wn * TN * 32 * 128;
        // Pinned order (r03, A/B in profiles/r03_split_gemm_notes.md): fragments of both 16-k sub-steps up front (the second set lands
        // while the first multiplies), the next stage's LDS-DMA loads spread behind the first MFMA groups instead of one burst
        frag_t fa[2][2][TM], fb[2][2][TN];
#pragma unroll
        for (int sb = 0; sb < 2; ++sb)
#pragma unroll
            for (int p = 0; p < 2; ++p) {
#pragma unroll
                for (int i = 0; i < TM; ++i) fa[sb][p][i] = *reinterpret_cast<const frag_t*>(a + i * 32 * 128 + fr_off[p][sb]);
#pragma unroll
                for (int j = 0; j < TN; ++j) fb[sb][p][j] = *reinterpret_cast<const frag_t*>(b + j * 32 * 128 + fr_off[p][sb]);
            }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int sb = 0; sb < 2; ++sb)
#pragma unroll
            for (int pr = 0; pr < 3; ++pr) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        if (ABL != 3) {
                            if constexpr (F16) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[sb][pr == 1 ? 1 : 0][i], fb[sb][pr == 0 ? 1 : 0][j], acc[i][j], 0, 0, 0);
                            else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[sb][pr == 1 ? 1 : 0][i], fb[sb][pr == 0 ? 1 : 0][j], acc[i][j], 0, 0, 0);
                        }
                        else acc[i][j][0] += (float)fa[sb][pr == 1 ? 1 : 0][i][0] * (float)fb[sb][pr == 0 ? 1 : 0][j][0];
                if (sb == 0 && ABL != 1 && more) issue_loads_part(buf ^ 1, pr);   // 3 + 3 + 2 loads behind the first three MFMA groups
                __builtin_amdgcn_sched_barrier(0);
            }
        __syncthreads();
    }
    flush(0);
}
// ---------------------------------------------------------------------------------------------------------------
// Three pieces on that structure: the exact-fp32 engine's deep component GEMMs (Winograd F(4x4,3x3) with Cin >= 512, polyphase F(4x4,2x2)).
// Operands: three bf16 planes, row-pair-interleaved (split3_layout.h: [row / 2][k / 32][row % 2][plane][32 k], 384-byte blocks = whole lines).
// Per 16-k sub-step and output tile the six products are accumulated SMALLEST FIRST, in this fixed order:
//     a0 b2, a1 b1, a2 b0   (<= 2^-18 |a b|),   a0 b1, a1 b0   (<= 2^-9 |a b|),   a0 b0
// i.e. the four smallest cross terms have gone into the accumulator before the two that carry 2^-9 |a b| and more; every product is exact,
// the accumulator rounds once per MFMA (f32), the dropped products a1 b2 + a2 b1 + a2 b2 are <= 3 * 2^-27 |a b|.
// Block tile 256 x 128, 8 waves of 64 x 64 (2 x 2 MFMA tiles), K-step 32, two LDS stages of (256 + 128) x 192 B = 72 KB: 384 MFMAs per CU and K-step, as
// many as the pair kernel's, for 72 KB of fill instead of 64.  One block per CU (144 KB of LDS), 2 waves per SIMD.
// Staging: a stage is 24 groups of 16 rows (16 of A, 8 of B), a group 3 LDS-DMA wave-loads (16 rows x 12 pieces of 16 B = 192 lane slots); wave w stages the
// A groups 4 (w / 2) + w % 2 and the one two further (the same 16 rows of the first and of the second 32 rows of a wave tile) and the B group w: 9 wave-loads per wave and K-step.  The LDS image of a group is lane-linear: slot = row * 12 + position, and a row's
// piece j = plane * 4 + (k / 8) sits at position (j + ((row >> 2) & 3)) mod 12 — the rotation goes on the per-lane SOURCE address and on the fragment reads
// (cdna_hip_programming.md rule 21).  With it the 16 rows of a ds_read_b128 lane group ({0-3, 12-15, 20-27} / {4-11, 16-19, 28-31} of a 32-row tile: every
// residue mod 16 once) land on 16 different 16-byte bank slots: 192-byte rows alone put them on four (12 r mod 16).
// The ring (profiles/split3_ring.md).  The two 72 KB stages are six units of 24 KB: of K-step t (stage t & 1) the unit A0(t) = the first 32 rows of every wave's
// 64 tile rows, A1(t) = the second 32, B(t) = the 128 column rows.  A wave stages one 16-row group (3 wave-loads) of each.  A K-step is two PHASES of 24 MFMAs per
// wave, each ended by s_waitcnt vmcnt (counted), s_waitcnt lgkmcnt(0) and a raw s_barrier.  Fragments live in two register sets, one per 16-k sub-step:
//     phase 0 of step t   multiplies tile row 0: sub-step 0 from set 0 (A0, B: read in the phase before), behind its first MFMA group reads sub-step 1 of A0(t), B(t)
//                         into set 1;  issues A1(t+1);  ends with vmcnt(3): A1(t) and A0, B(t+1) have landed, A1(t+1) stays in flight  (vmcnt(0) in the last step)
//     phase 1 of step t   multiplies tile row 1 against the same B fragments: reads sub-step 0 of A1(t) (the only reads no MFMA covers), then sub-step 1 behind the
//                         first group, and behind the first group of sub-step 1 reads sub-step 0 of A0(t+1), B(t+1) into set 0 for the next phase;  issues A0(t+2),
//                         B(t+2);  ends with no vmcnt wait at all: those six and A1(t+1) stay in flight
// A unit is restaged one phase after the phase that last read it (A1(t+1) overwrites A1(t-1), read in phase 1 of t-1; A0 / B(t+2) overwrite A0 / B(t), last read in
// phase 0 of t; every read has returned before its phase's barrier: lgkmcnt(0)) and is first read in a phase after the wait + barrier that retired it.  Every unit
// has two phases of matrix work to land under, and nine / three wave-loads per wave are in flight across the barriers; with __syncthreads() (vmcnt(0)) a stage
// had less than one K-step and nothing crossed a barrier.  Every wave issues the same number of loads per phase: the counts are constants for all waves.
// A phase's loads go out one per MFMA group, and the two waves of a SIMD (w and w + 4), which leave every barrier in step, issue theirs in different sub-steps:
// while one waits for the vector-memory pipe to take a load the other multiplies.  That stagger is what moved the K loop's slope (0.193 -> 0.18 ms per 512 of
// K); the span alone moved the fixed cost.  While an LDS-DMA is pending the compiler turns every wait for a fragment into lgkmcnt(0), so a read is placed behind
// the MFMA group in front of which the previous reads are waited for (sched_barrier pins that), never in front of it.
// Operand layout, LDS image, rotation and global access (whole 384-byte row-pair blocks) are unchanged, which is why the ring is cut by tile ROW and not into
// 16-k half-stages: those need the operands re-laid at 16-k granularity in every writer to keep whole-line traffic, and leave 4.5 wave-loads per wave and
// half-stage.  Per output element: the same six products per 16-k sub-step in the same order over the same K order.
// DRAIN = true (the twin: irsde_debug_split_gemm 47, IRSDE_SPLIT3_DRAIN=1) waits vmcnt(0) in front of every barrier: same issue order, same bits, no span.
// ---------------------------------------------------------------------------------------------------------------
// WALK (the production launch): at most one block per CU, and a block walks several items (component, row tile, column tile) as ONE pipelined loop.  The
// items of an XCD (its units in order, column tiles innermost) are dealt round-robin to the XCD's blocks: block j of nb takes items j, j + nb, j + 2 nb ...,
// so at any time the blocks of an XCD work on neighbouring items (the column tiles of a unit side by side, as the one-item launch's dispatch order has them)
// and an A row tile is still read through one L2.  The map is a pure function of the shape and the grid: no atomics, graph replay = eager launches.
// At an item boundary both LDS stages are free behind the barrier that ended the last K-step and nothing is in flight: the next item's first LDS-DMA loads
// (step 0 and A0, B of step 1; no VGPRs) are issued BEFORE the finished accumulators are stored, so their HBM / L2 latency runs under the 64 stores per wave,
// and the item opens with a full drain (vmcnt(0): the counter holds the stores too, which do not retire in order with loads) and a barrier.  Per output
// element nothing changes: WALK = false, the one-item-per-block launch, is the bit-identity twin (irsde_debug_split_gemm 45, IRSDE_SPLIT3_WALK=0).
#define IRSDE_WAIT_VM(N) asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory")
#define IRSDE_PHASE_BARRIER()                              \
    do {                                                   \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); \
        __builtin_amdgcn_s_barrier();                      \
    } while (0)
template <int ABL = 0, bool WALK = true, bool DRAIN = false>
__global__ __launch_bounds__(512, 1) void gemm_split3i_kernel(const SplitGemmArgs g) {
    constexpr int TM = 2, TN = 2, WN = 2, BM = 256, BN = 128;
    constexpr int ROWB = 192, GROUP = 16 * ROWB;                       // bytes per LDS row (12 pieces) and per 16-row group
    constexpr int A_STAGE = BM * ROWB, STAGE = (BM + BN) * ROWB;       // bytes
    // smallest products first (see above): plane of A, plane of B
    constexpr int PA[6] = {0, 1, 2, 0, 1, 0};
    constexpr int PB[6] = {2, 1, 0, 1, 0, 0};
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, h = lane >> 5;
    // XCD-contiguous (component, row tile) units with all their column tiles side by side, as in gemm_split2i_kernel
    const int mtiles = (g.M + BM - 1) / BM;
    const int units = mtiles * g.n_inner;          // (n_inner carries the component count here)
    const int xcd = blockIdx.x & 7, jx = blockIdx.x >> 3;
    const int ulo = (int)((long long)xcd * units / 8), uhi = (int)((long long)(xcd + 1) * units / 8);
    const int nitems = (uhi - ulo) * g.nblk_n;     // this XCD's items: (unit, column tile), column tiles innermost
    const int it_step = WALK ? ((int)gridDim.x - xcd + 7) >> 3 : nitems;   // blocks of this launch on this XCD (WALK = false: one item per block)
    int it = jx;
    if (it >= nitems) return;
    const int nk = g.K / SG_BK;
    const unsigned pairb = (unsigned)nk * 384u;   // bytes per operand row pair: K / 32 blocks of 2 rows x 3 planes x 64 B

    // staging: the wave's 16-row groups: of A0 group 4 (w / 2) + w % 2 (rows 64 (w / 2) + 16 (w % 2) ...), of A1 the group two further (32 rows on), of B group w.
    // Lane slot s = wl * 64 + lane of a group = (row s / 12, position s % 12); the lane fetches the row's piece (position - rotation) mod 12.
    // Rows past M / N are clamped: they feed accumulator rows / columns that are never stored.
    const int ga0 = 4 * (wave >> 1) + (wave & 1);
    int plane0, m0, n0;
    unsigned a_voff[6], b_voff[3];
    const char *acomp, *bcomp;
    auto set_item = [&](int i) {
        const int unit = ulo + i / g.nblk_n, nblk = i % g.nblk_n;
        plane0 = unit / mtiles;
        m0 = (unit - plane0 * mtiles) * BM;
        n0 = nblk * BN;
#pragma unroll
        for (int q = 0; q < 9; ++q) {
            const int gi = q / 3, wl = q - gi * 3;     // gi 0: the wave's A0 group, 1: its A1 group, 2: its B group
            const int sl = wl * 64 + lane;
            const int r = sl / 12, pos = sl - r * 12;
            int j = pos - ((r >> 2) & 3);
            j = j < 0 ? j + 12 : j;
            if (gi < 2) {
                int m = m0 + (ga0 + 2 * gi) * 16 + r;
                m = m < g.M ? m : g.M - 1;
                a_voff[q] = (unsigned)(m >> 1) * pairb + (unsigned)(m & 1) * 192u + (unsigned)j * 16u;
            } else {
                int n = n0 + wave * 16 + r;
                n = n < g.N ? n : g.N - 1;
                b_voff[wl] = (unsigned)(n >> 1) * pairb + (unsigned)(n & 1) * 192u + (unsigned)j * 16u;
            }
        }
        acomp = reinterpret_cast<const char*>(g.a) + (long long)plane0 * g.pA * 2;   // pA / pB: unsigned shorts per component
        bcomp = reinterpret_cast<const char*>(g.b) + (long long)plane0 * g.pB * 2;
    };
    auto issue_unit = [&](int kb, int kind) {   // the wave's 3 loads of a unit of K-step kb (stage kb & 1): kind 0 = A0, 1 = A1, 2 = B
        const char* gsrc = (kind < 2 ? acomp : bcomp) + (size_t)kb * 384;
        char* l = lds + (kb & 1) * STAGE + (kind < 2 ? (ga0 + 2 * kind) * GROUP : A_STAGE + wave * GROUP);
#pragma unroll
        for (int wl = 0; wl < 3; ++wl) IRSDE_GLDS16(gsrc + (kind < 2 ? a_voff[kind * 3 + wl] : b_voff[wl]), l + wl * 1024);
    };
    auto issue_one = [&](int kb, int kind, int wl) {   // one of those loads
        const char* gsrc = (kind < 2 ? acomp : bcomp) + (size_t)kb * 384;
        char* l = lds + (kb & 1) * STAGE + (kind < 2 ? (ga0 + 2 * kind) * GROUP : A_STAGE + wave * GROUP);
        IRSDE_GLDS16(gsrc + (kind < 2 ? a_voff[kind * 3 + wl] : b_voff[wl]), l + wl * 1024);
    };
    auto issue_first = [&]() {   // an item's opening loads, in the ring's order: A0, B, A1 of step 0, then A0, B of step 1
        issue_unit(0, 0);
        issue_unit(0, 2);
        issue_unit(0, 1);
        if (nk > 1) {
            issue_unit(1, 0);
            issue_unit(1, 2);
        }
    };

    floatx16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    set_item(it);
    issue_first();

    // fragment offsets: row l31 of a 32-row tile (two 16-row groups back to back = 192 bytes per row), piece plane * 4 + sb * 2 + h, rotated by (row >> 2) & 3
    int fr_off[3][2];
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int sb = 0; sb < 2; ++sb) fr_off[p][sb] = l31 * ROWB + ((p * 4 + sb * 2 + h + ((l31 >> 2) & 3)) % 12) * 16;
    // fragment sets: [sb] = the 16-k sub-step; fb holds the B fragments of a K-step through both phases
    bf16x8 fa[2][3], fb[2][3][TN];
    auto read_a = [&](int sb, const char* a) {
#pragma unroll
        for (int p = 0; p < 3; ++p) fa[sb][p] = *reinterpret_cast<const bf16x8*>(a + fr_off[p][sb]);
    };
    auto read_b = [&](int sb, const char* b) {
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[sb][p][j] = *reinterpret_cast<const bf16x8*>(b + j * 32 * ROWB + fr_off[p][sb]);
    };
    const bool late = wave >= 4;
    const int a_base = wm * TM * 32 * ROWB, b_base = A_STAGE + wn * TN * 32 * ROWB;
    for (;;) {
        IRSDE_WAIT_VM(0);   // the item's opening loads have landed (and, behind an earlier item, that item's stores have left)
        IRSDE_PHASE_BARRIER();
        read_a(0, lds + a_base);   // sub-step 0 of step 0: the only fragment reads of an item that no MFMA covers
        read_b(0, lds + b_base);
        __builtin_amdgcn_sched_barrier(0);
        for (int st = 0; st < nk; ++st) {
            const bool more1 = st + 1 < nk, more2 = st + 2 < nk;
            const char* a = lds + (st & 1) * STAGE + a_base;
            const char* b = lds + (st & 1) * STAGE + b_base;
            const char* an = lds + ((st + 1) & 1) * STAGE + a_base;
            const char* bn = lds + ((st + 1) & 1) * STAGE + b_base;
#pragma unroll
            for (int i = 0; i < TM; ++i) {   // phase i: tile row i
                if (i == 1) {
                    read_a(0, a + 32 * ROWB);
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int sb = 0; sb < 2; ++sb)
#pragma unroll
                    for (int pr = 0; pr < 6; ++pr) {
#pragma unroll
                        for (int j = 0; j < TN; ++j) {
                            if (ABL != 3) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[sb][PA[pr]], fb[sb][PB[pr]][j], acc[i][j], 0, 0, 0);
                            else acc[i][j][0] += (float)fa[sb][PA[pr]][0] * (float)fb[sb][PB[pr]][j][0];
                        }
                        __builtin_amdgcn_sched_barrier(0);
                        // fragment reads a whole sub-step ahead of their first use, behind the first MFMA group of the sub-step that covers them (the
                        // compiler waits lgkmcnt(0) at the first use of any fragment while an LDS-DMA is pending: reads issued before that group would be waited for)
                        if (sb == 0 && pr == 0) {
                            if (i == 0) {
                                read_a(1, a);
                                read_b(1, b);
                            } else {
                                read_a(1, a + 32 * ROWB);
                            }
                        }
                        if (i == 1 && sb == 1 && pr == 0 && more1) {   // sub-step 0 of the next step: A0, B(st + 1) were retired at the end of phase 0
                            read_a(0, an);
                            read_b(0, bn);
                        }
                        // the phase's loads one per MFMA group; the two waves of a SIMD (w and w + 4 leave a barrier in step) issue theirs in different sub-steps,
                        // so that one of them multiplies while the other waits for the vector-memory pipe to take its load
                        if (ABL != 1 && (sb == 1) == late) {
                            if (i == 0 && pr >= 1 && pr <= 3 && more1) issue_one(st + 1, 1, pr - 1);
                            if (i == 1 && more2) issue_one(st + 2, pr < 3 ? 0 : 2, pr % 3);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                // phase 0 retires A1(st) and A0, B(st + 1) and leaves A1(st + 1) in flight; phase 1 retires nothing and leaves that and A0, B(st + 2) in flight
                if (DRAIN || (i == 0 && !more1)) IRSDE_WAIT_VM(0);
                else if (i == 0) IRSDE_WAIT_VM(3);
                IRSDE_PHASE_BARRIER();
            }
        }

        // registers -> buffer stores: rows past M dropped by the descriptor, columns past N masked
        const int rowb_ = m0 + wm * TM * 32, colb = n0 + wn * TN * 32;
        float* ob = g.out + (long long)plane0 * g.pO + (long long)rowb_ * g.ldc;
        const int rows = g.M - rowb_;
        const unsigned nrec = rows <= 0 ? 0u : (unsigned)(rows < TM * 32 ? rows : TM * 32) * (unsigned)g.ldc * 4u;
        const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(ob, 0, nrec, 0x00020000);
        it += it_step;
        const bool next = WALK && it < nitems;
        if (next) {   // both stages are free behind the last step's barrier: the next item's opening loads go out ahead of this item's stores
            set_item(it);
            issue_first();
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int colu = colb + j * 32;
                if (colu + l31 < g.N && (ABL != 4 || acc[i][j][0] == 1.2345e30f)) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float v = acc[i][j][r];
                        // (the whole offset in the vector operand: that is the part the descriptor's range check is sure to cover)
                        const unsigned voff = (unsigned)((i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * g.ldc + colu + l31) * 4u;
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ro, (int)voff, 0, 0);
                    }
                }
            }
        if (!next) break;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    }
}
// ---------------------------------------------------------------------------------------------------------------
// The plain 1x1 convolutions on three pieces ("a" = the A operand is an ordinary f32 activation tensor, split INSIDE the kernel; profiles/split3_1x1.md):
//     out[m][n] = sum_k A[m][k] W[n][k] (+ bias[n]),   A = up to two f32 NHWC sources side by side (the never-materialised concat [x | skip]),
// W = the triples of split_triples_kernel (split3_layout.h), exactly gemm_split3i_kernel's B operand.  A separate triple writer for A would add an HBM pass of
// 6 bytes per element, more than the GEMM saves: the raw f32 rows go to LDS by LDS-DMA instead, and a wave splits its own fragment in registers
// (hi = RNE bf16(x), mid = RNE bf16(x - hi), lo = RNE bf16(x - hi - mid): split_triples_kernel's chain) and feeds the three planes straight to the MFMAs.
// Per output element: the six products of a 16-k sub-step in gemm_split3i_kernel's order, over the same K order, with the same k -> lane assignment (lane
// (row l31, h) holds k = 16 sb + 8 h .. + 7), so the result is BIT-IDENTICAL to split_triples_kernel on A followed by gemm_split3i_kernel.
// Block tile 256 x 128, 8 waves of 32 rows x all 128 columns (1 x 4 MFMA tiles): every A element is split once per column tile, and there is no LDS write of
// pieces.  A wave reads per K-step 4 KB of A and the 24 KB of B: 28 KB, against gemm_split3i's 24.
// LDS: two stages of A 256 rows x 128 B (raw f32; 16-byte pieces XOR-swizzled by (row >> 1) & 7 on the SOURCE address, gemm_split2i's image) + B 128 rows x
// 192 B (gemm_split3i's image and rotation) = 56 KB.
// The ring is gemm_split3i's with the operands' roles swapped: the two PHASES of a K-step are the two column halves (64 columns = 2 MFMA tiles, 24 MFMAs per
// wave), the A fragments of a K-step stay in registers through both.  Units: A(t) 32 KB = 4 wave-loads per wave, B0(t) / B1(t) = the 64 rows of a column half,
// 12 KB = 96 lane slots per wave: 2 wave-loads, the second over slots 32 .. 95 (it fetches slots 32 .. 63 again: every wave issues whole wave-loads and the
// counts are the same constants for all waves).
//     phase 0 of step t   multiplies columns 0 - 63: sub-step 0 from set 0 (read in the phase before), reads sub-step 1 of A(t), B0(t) behind its first MFMA
//                         group and splits A three groups later; issues B1(t+1) (2 loads); ends with vmcnt(2): B1(t), A(t+1), B0(t+1) have landed
//                         (vmcnt(0) in the last step)
//     phase 1 of step t   multiplies columns 64 - 127 against the same A pieces: reads sub-step 0 of B1(t) (uncovered: B1(t) is retired only at the end of
//                         phase 0, so once per K-step the matrix pipe waits for an LDS read), sub-step 1 behind the first group, and behind the
//                         first group of sub-step 1 sub-step 0 of A(t+1), B0(t+1) (split three groups later); issues A(t+2), B0(t+2) (6 loads); no vmcnt wait
// A unit is restaged one phase after the phase that last read it and first read one phase after the wait + barrier that retired it, as there.
// WALK / DRAIN: the same twins (irsde_debug_split3_1x1 modes 1 / 2).  The bias is loaded at an item's opening, in front of its LDS-DMA loads, and is retired
// by the opening's vmcnt(0): no ordinary load is pending while the ring runs.
template <int ABL = 0, bool WALK = true, bool DRAIN = false>
__global__ __launch_bounds__(512, 1) void gemm_split3a_kernel(const Split3aArgs g) {
    constexpr int TN = 4, BM = 256, BN = 128;
    constexpr int AROW = 128, BROW = 192;                                           // bytes per LDS row: 32 f32 of A, 12 pieces of B
    constexpr int A_STAGE = BM * AROW, B_HALF = 64 * BROW, STAGE = A_STAGE + 2 * B_HALF;   // bytes
    constexpr int PA[6] = {0, 1, 2, 0, 1, 0};
    constexpr int PB[6] = {2, 1, 0, 1, 0, 0};
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    // XCD-contiguous row tiles with their column tiles side by side; the walk deals an XCD's items round-robin to its blocks (gemm_split3i_kernel)
    const int units = (g.M + BM - 1) / BM;
    const int xcd = blockIdx.x & 7, jx = blockIdx.x >> 3;
    const int ulo = (int)((long long)xcd * units / 8), uhi = (int)((long long)(xcd + 1) * units / 8);
    const int nitems = (uhi - ulo) * g.nblk_n;
    const int it_step = WALK ? ((int)gridDim.x - xcd + 7) >> 3 : nitems;
    int it = jx;
    if (it >= nitems) return;
    const int nk0 = g.C0 / SG_BK, nk = (g.C0 + g.C1) / SG_BK;
    const unsigned pairb = (unsigned)nk * 384u;   // bytes per row pair of W

    // staging.  A: wave-load ps = the 8 rows of chunk ps * 8 + wave, lane = (row lane / 8, slot lane % 8) fetches the row's piece slot ^ ((row >> 1) & 7).
    // B half hb: the wave's rows 8 wave .. + 7 of the half, lane slot s = (row s / 12, position s % 12), wave-load 0 = slots 0 .. 63, 1 = slots 32 .. 95.
    // Rows past M / N are clamped: they feed accumulator rows / columns that are never stored.
    int m0, n0;
    unsigned a_voff0[4], a_voff1[4], b_voff[2][2];
    float bias_r[TN];
    auto set_item = [&](int i) {
        const int unit = ulo + i / g.nblk_n, nblk = i % g.nblk_n;
        m0 = unit * BM;
        n0 = nblk * BN;
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) {
            const int row = (ps * 8 + wave) * 8 + (lane >> 3);
            const unsigned pc = (unsigned)((lane & 7) ^ ((row >> 1) & 7)) * 16u;
            int m = m0 + row;
            m = m < g.M ? m : g.M - 1;
            a_voff0[ps] = (unsigned)m * (unsigned)g.pix0 * 4u + pc;
            a_voff1[ps] = (unsigned)m * (unsigned)g.pix1 * 4u + pc;
        }
#pragma unroll
        for (int hb = 0; hb < 2; ++hb)
#pragma unroll
            for (int wl = 0; wl < 2; ++wl) {
                const int sl = wl * 32 + lane;
                const int r = sl / 12, pos = sl - r * 12;
                const int rowt = wave * 8 + r;
                int j = pos - ((rowt >> 2) & 3);
                j = j < 0 ? j + 12 : j;
                int n = n0 + hb * 64 + rowt;
                n = n < g.N ? n : g.N - 1;
                b_voff[hb][wl] = (unsigned)(n >> 1) * pairb + (unsigned)(n & 1) * 192u + (unsigned)j * 16u;
            }
        if (g.bias) {
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                int n = n0 + j * 32 + l31;
                n = n < g.N ? n : g.N - 1;
                bias_r[j] = g.bias[n];
            }
        }
    };
    auto issue_a = [&](int kb, int ps) {   // one of the wave's 4 loads of A(kb)
        const bool second = kb >= nk0;
        const char* gsrc = second ? reinterpret_cast<const char*>(g.in1) + (size_t)(kb - nk0) * 128 : reinterpret_cast<const char*>(g.in0) + (size_t)kb * 128;
        IRSDE_GLDS16(gsrc + (second ? a_voff1[ps] : a_voff0[ps]), lds + (kb & 1) * STAGE + (ps * 8 + wave) * 1024);
    };
    auto issue_b = [&](int kb, int hb, int wl) {   // one of the wave's 2 loads of column half hb of B(kb)
        const char* gsrc = reinterpret_cast<const char*>(g.w3) + (size_t)kb * 384;
        IRSDE_GLDS16(gsrc + b_voff[hb][wl], lds + (kb & 1) * STAGE + A_STAGE + hb * B_HALF + wave * 8 * BROW + wl * 512);
    };
    auto issue_first = [&]() {   // an item's opening loads, in the ring's order: B0, A, B1 of step 0, then A, B0 of step 1
        issue_b(0, 0, 0); issue_b(0, 0, 1);
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) issue_a(0, ps);
        issue_b(0, 1, 0); issue_b(0, 1, 1);
        if (nk > 1) {
#pragma unroll
            for (int ps = 0; ps < 4; ++ps) issue_a(1, ps);
            issue_b(1, 0, 0); issue_b(1, 0, 1);
        }
    };

    floatx16 acc[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    set_item(it);
    issue_first();

    // fragment offsets.  A: row l31 of the wave's 32, the two 16-byte pieces 2 q, 2 q + 1 of k block q = 2 sb + h, swizzled.  B: as gemm_split3i_kernel.
    const int swz = (l31 >> 1) & 7;
    int fa_off[2][2], fr_off[3][2];
#pragma unroll
    for (int sb = 0; sb < 2; ++sb)
#pragma unroll
        for (int e = 0; e < 2; ++e) fa_off[sb][e] = l31 * AROW + (((2 * (2 * sb + h) + e) ^ swz) * 16);
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int sb = 0; sb < 2; ++sb) fr_off[p][sb] = l31 * BROW + ((p * 4 + sb * 2 + h + ((l31 >> 2) & 3)) % 12) * 16;
    // fragment sets: [sb] = the 16-k sub-step; fa holds the A pieces of a K-step through both phases, ra the raw f32 of the sub-step read last
    bf16x8 fa[2][3], fb[2][3][2];
    floatx4 ra[2];
    auto read_a = [&](int sb, const char* a) {
#pragma unroll
        for (int e = 0; e < 2; ++e) ra[e] = *reinterpret_cast<const floatx4*>(a + fa_off[sb][e]);
    };
    auto split_a = [&](int sb) {   // split_triples_kernel's chain: every residual is exact in f32
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float r = ra[e >> 2][e & 3];
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                const __bf16 hb = (__bf16)r;
                fa[sb][p][e] = hb;
                r -= (float)hb;
            }
        }
    };
    auto read_b = [&](int sb, const char* b) {
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[sb][p][j] = *reinterpret_cast<const bf16x8*>(b + j * 32 * BROW + fr_off[p][sb]);
    };
    const bool late = wave >= 4;
    const int a_base = wave * 32 * AROW;
    for (;;) {
        IRSDE_WAIT_VM(0);   // the item's opening loads and its bias have landed (and, behind an earlier item, that item's stores have left)
        IRSDE_PHASE_BARRIER();
        read_a(0, lds + a_base);   // sub-step 0 of step 0: no MFMA covers these reads (nor, in every K-step, phase 1's read of sub-step 0 of B1 below)
        read_b(0, lds + A_STAGE);
        split_a(0);
        __builtin_amdgcn_sched_barrier(0);
        for (int st = 0; st < nk; ++st) {
            const bool more1 = st + 1 < nk, more2 = st + 2 < nk;
            const char* a = lds + (st & 1) * STAGE + a_base;
            const char* b = lds + (st & 1) * STAGE + A_STAGE;
            const char* an = lds + ((st + 1) & 1) * STAGE + a_base;
            const char* bn = lds + ((st + 1) & 1) * STAGE + A_STAGE;
#pragma unroll
            for (int i = 0; i < 2; ++i) {   // phase i: column half i
                if (i == 1) {   // B1(st) was retired by the wait + barrier that ended phase 0: its sub-step 0 cannot be read earlier, and no MFMA covers the read
                    read_b(0, b + B_HALF);
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int sb = 0; sb < 2; ++sb)
#pragma unroll
                    for (int pr = 0; pr < 6; ++pr) {
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            if (ABL != 3) acc[2 * i + j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[sb][PA[pr]], fb[sb][PB[pr]][j], acc[2 * i + j], 0, 0, 0);
                            else acc[2 * i + j][0] += (float)fa[sb][PA[pr]][0] * (float)fb[sb][PB[pr]][j][0];
                        }
                        __builtin_amdgcn_sched_barrier(0);
                        // fragment reads a whole sub-step ahead of their first use, behind the first MFMA group of the sub-step that covers them; the raw A
                        // values are split three groups later, when they have arrived
                        if (sb == 0 && pr == 0) {
                            if (i == 0) {
                                read_a(1, a);
                                read_b(1, b);
                            } else {
                                read_b(1, b + B_HALF);
                            }
                        }
                        if (i == 0 && sb == 0 && pr == 3) split_a(1);
                        if (i == 1 && sb == 1 && more1) {   // sub-step 0 of the next step: A, B0(st + 1) were retired at the end of phase 0
                            if (pr == 0) {
                                read_a(0, an);
                                read_b(0, bn);
                            }
                            if (pr == 3) split_a(0);
                        }
                        // the phase's loads one per MFMA group; the two waves of a SIMD (w and w + 4) issue theirs in different sub-steps
                        if (ABL != 1 && (sb == 1) == late) {
                            if (i == 0 && pr >= 1 && pr <= 2 && more1) issue_b(st + 1, 1, pr - 1);
                            if (i == 1 && more2) {
                                if (pr < 4) issue_a(st + 2, pr);
                                else issue_b(st + 2, 0, pr - 4);
                            }
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                // phase 0 retires B1(st) and A, B0(st + 1) and leaves B1(st + 1) in flight; phase 1 retires nothing and leaves that and A, B0(st + 2) in flight
                if (DRAIN || (i == 0 && !more1)) IRSDE_WAIT_VM(0);
                else if (i == 0) IRSDE_WAIT_VM(2);
                IRSDE_PHASE_BARRIER();
            }
        }

        // + bias, then registers -> buffer stores: rows past M dropped by the descriptor, columns past N masked
        if (g.bias) {
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][r] += bias_r[j];
        }
        const int rowb_ = m0 + wave * 32, colb = n0;
        float* ob = g.out + (long long)rowb_ * g.out_stride;
        const int rows = g.M - rowb_;
        const unsigned nrec = rows <= 0 ? 0u : (unsigned)(rows < 32 ? rows : 32) * (unsigned)g.out_stride * 4u;
        const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(ob, 0, nrec, 0x00020000);
        it += it_step;
        const bool next = WALK && it < nitems;
        if (next) {   // both stages are free behind the last step's barrier: the next item's opening loads go out ahead of this item's stores
            __builtin_amdgcn_sched_barrier(0);
            set_item(it);
            issue_first();
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int colu = colb + j * 32;
            if (colu + l31 < g.N && (ABL != 4 || acc[j][0] == 1.2345e30f)) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float v = acc[j][r];   // (a copy: __builtin_bit_cast on the vector element itself reads element 0)
                    const unsigned voff = (unsigned)(((r & 3) + 8 * (r >> 2) + 4 * h) * g.out_stride + colu + l31) * 4u;
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ro, (int)voff, 0, 0);
                }
            }
        }
        if (!next) break;
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    }
}
#undef IRSDE_PHASE_BARRIER
#undef IRSDE_WAIT_VM
#undef IRSDE_GLDS16

// f32 [ncomp][rows][K] -> the three-piece row-pair-interleaved layout (split3_layout.h)
__global__ __launch_bounds__(256) void split_triples_kernel(const float* __restrict__ in, unsigned short* __restrict__ out, const size_t n, const size_t rows,
                                                            const int K) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t rk = rows * (size_t)K;
    const size_t z = i / rk, rem = i - z * rk;
    const size_t row = rem / K;
    const int k = (int)(rem - row * K);
    float r = in[i];
    unsigned short* o = out + z * split3_comp_elems(rows, K);
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        const __bf16 hb = (__bf16)r;
        o[split3_index(row, k, p, K / 32)] = __builtin_bit_cast(unsigned short, hb);
        r -= (float)hb;
    }
}

// f32 -> pair-interleaved hi / lo pieces: element (row, k) of a [rows][K] matrix -> out[(row * K / 32 + k / 32) * 64 + plane * 32 + k % 32].
// F16: the pieces are IEEE binary16 of in * scale (scale = a power of two that brings the tensor into fp16's range).
template <bool F16>
__global__ __launch_bounds__(256) void split_pairs_kernel(const float* __restrict__ in, unsigned short* __restrict__ out, const size_t n, const int K,
                                                          const float scale) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t row = i / K;
    const int k = (int)(i - row * K);
    float r = in[i];
    const size_t base = (row * (size_t)(K / 32) + k / 32) * 64 + (k & 31);
    if constexpr (F16) {
        r *= scale;
        const _Float16 hb = (_Float16)r;
        out[base] = __builtin_bit_cast(unsigned short, hb);
        r -= (float)hb;
        const _Float16 lb = (_Float16)r;
        out[base + 32] = __builtin_bit_cast(unsigned short, lb);
    } else {
        const __bf16 hb = (__bf16)r;
        out[base] = __builtin_bit_cast(unsigned short, hb);
        r -= (float)hb;
        const __bf16 lb = (__bf16)r;
        out[base + 32] = __builtin_bit_cast(unsigned short, lb);
    }
}

// f32 -> NPL bf16 planes (round to nearest even; every residual is exact in f32); F16: IEEE fp16 pieces of in * scale
template <int NPL, bool F16 = false>
__global__ __launch_bounds__(256) void split_planes_kernel(const float* __restrict__ in, unsigned short* __restrict__ out, const size_t n,
                                                           const size_t plane, const float scale) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float r = F16 ? in[i] * scale : in[i];
#pragma unroll
    for (int p = 0; p < NPL; ++p) {
        if constexpr (F16) {
            const _Float16 hb = (_Float16)r;
            out[p * plane + i] = __builtin_bit_cast(unsigned short, hb);
            r -= (float)hb;
        } else {
            const __bf16 hb = (__bf16)r;
            out[p * plane + i] = __builtin_bit_cast(unsigned short, hb);
            r -= (float)hb;
        }
    }
}

// f32 [rows][K] -> three bf16 planes in MFMA-fragment order (the fused attention kernels' three-piece weights, attn_frag3_index in common.h): the 64 x 16 bytes
// one wave loads as the operand of v_mfma_f32_32x32x16_bf16 for (32-row tile, 16-k step) are one contiguous KB, so every line fetched from L2 is used whole
__global__ __launch_bounds__(256) void split_frag3_kernel(const float* __restrict__ in, unsigned short* __restrict__ out, const size_t n, const int K) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t row = i / K;
    const int k = (int)(i - row * K);
    float r = in[i];
    const size_t o = attn_frag3_index(row, k, K);
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        const __bf16 hb = (__bf16)r;
        out[p * n + o] = __builtin_bit_cast(unsigned short, hb);
        r -= (float)hb;
    }
}

}  // namespace

void launch_split_frag3(const float* in, unsigned short* out, size_t rows, int K, hipStream_t s) {
    if (rows % 32 || K % 16) throw HipError("split_frag3: rows must be a multiple of 32, K of 16");
    const size_t n = rows * (size_t)K;
    hipLaunchKernelGGL(split_frag3_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, out, n, K);
    IRSDE_HIP_CHECK(hipGetLastError());
}

void gemm_split_global_init() {
    IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_split2i_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_split2i_kernel<0, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_split2i_kernel<5, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_split2i_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_split2i_kernel<3>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_split2i_kernel<4>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_split3i_kernel<0, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_split3i_kernel<0, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_split3i_kernel<0, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_split3a_kernel<0, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_split3a_kernel<0, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_split3a_kernel<0, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
#ifdef IRSDE_PROBES
    for (const void* f : {reinterpret_cast<const void*>(gemm_split3a_kernel<1, true>), reinterpret_cast<const void*>(gemm_split3a_kernel<3, true>),
                          reinterpret_cast<const void*>(gemm_split3a_kernel<4, true>), reinterpret_cast<const void*>(gemm_split3a_kernel<1, false>),
                          reinterpret_cast<const void*>(gemm_split3a_kernel<3, false>), reinterpret_cast<const void*>(gemm_split3a_kernel<4, false>),
                          reinterpret_cast<const void*>(gemm_split3a_kernel<1, true, true>), reinterpret_cast<const void*>(gemm_split3a_kernel<3, true, true>),
                          reinterpret_cast<const void*>(gemm_split3a_kernel<4, true, true>)})
        IRSDE_HIP_CHECK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_split3i_kernel<1, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_split3i_kernel<3, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_split3i_kernel<4, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_split3i_kernel<1, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_split3i_kernel<3, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_split3i_kernel<4, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_split3i_kernel<1, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_split3i_kernel<3, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_split3i_kernel<4, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
#endif
}

// pair-interleaved operands (g.a / g.b in the [row][k/32][plane][32] layout, g.pA / g.pB = elements per component and plane)
void launch_gemm_split_pairs(const SplitGemmArgs& a, int ncomp, hipStream_t s, int abl, bool f16) {
    if (a.K % SG_BK) throw HipError("gemm_split_pairs: K must be a multiple of 32");
    if ((unsigned long long)a.M * a.K * 4ull >= 0xffffffffull || (unsigned long long)a.N * a.K * 4ull >= 0xffffffffull ||
        (size_t)a.M * a.ldc * 4 >= 0xffffffffull)
        throw HipError("gemm_split_pairs: a component exceeds the 32-bit offset range");
    SplitGemmArgs g = a;
    g.nblk_n = (a.N + 255) / 256;
    g.n_inner = ncomp;   // this kernel: one (component, row tile, column tile) per block; n_inner carries the component count
    const int units = ((a.M + 255) / 256) * ncomp;
    int per_xcd = 0;
    for (int x = 0; x < 8; ++x) per_xcd = std::max(per_xcd, (int)((long long)(x + 1) * units / 8) - (int)((long long)x * units / 8));
    const dim3 grid((unsigned)(8 * per_xcd * g.nblk_n));
    const size_t lds = (size_t)2 * 512 * 128;
    if (f16) {
        if (abl != 0) throw HipError("gemm_split_pairs: the ablation twins exist for the bf16 kernel only");
        static const bool nt = tuning_env_int("IRSDE_SPLIT_NT", 0) != 0;
        if (nt) hipLaunchKernelGGL((gemm_split2i_kernel<5, true>), grid, dim3(512), lds, s, g);
        else hipLaunchKernelGGL((gemm_split2i_kernel<0, true>), grid, dim3(512), lds, s, g);
        IRSDE_HIP_CHECK(hipGetLastError());
        return;
    }
    switch (abl) {
        case 0: hipLaunchKernelGGL(gemm_split2i_kernel<0>, grid, dim3(512), lds, s, g); break;
        case 1: hipLaunchKernelGGL(gemm_split2i_kernel<1>, grid, dim3(512), lds, s, g); break;
        case 3: hipLaunchKernelGGL(gemm_split2i_kernel<3>, grid, dim3(512), lds, s, g); break;
        case 4: hipLaunchKernelGGL(gemm_split2i_kernel<4>, grid, dim3(512), lds, s, g); break;
        default: throw HipError("gemm_split_pairs: bad ablation variant");
    }
    IRSDE_HIP_CHECK(hipGetLastError());
}

bool gemm_split_triples_fits(long long M, long long N, long long K, long long ldc) {
    if (M < 1 || N < 1 || K < 32 || K % SG_BK) return false;
    return (unsigned long long)split3_comp_elems((size_t)M, (size_t)K) * 2ull < 0xffffffffull && (unsigned long long)split3_comp_elems((size_t)N, (size_t)K) * 2ull < 0xffffffffull &&
           (unsigned long long)M * ldc * 4ull < 0xffffffffull;
}

static std::atomic<int> g_force_split3_blocks{-1};   // irsde_debug_force_split3_blocks: -1 = one block per CU
void set_force_split3_blocks(int n) { g_force_split3_blocks.store(n >= 8 ? n : -1, std::memory_order_relaxed); }

// three-piece row-pair-interleaved operands (split3_layout.h; g.pA / g.pB = unsigned shorts per component)
// o.walk: at most one block per CU (or the forced cap), each walking its share of the items / one item per block (the twin)
// o.drain: the walk's drain twin (vmcnt(0) in front of every barrier of the K loop) / the ring
template <int ABL>
static void launch_split3_abl(bool walk, bool drain, dim3 grid, size_t lds, hipStream_t s, const SplitGemmArgs& g) {
    if (drain) hipLaunchKernelGGL((gemm_split3i_kernel<ABL, true, true>), grid, dim3(512), lds, s, g);
    else if (walk) hipLaunchKernelGGL((gemm_split3i_kernel<ABL, true>), grid, dim3(512), lds, s, g);
    else hipLaunchKernelGGL((gemm_split3i_kernel<ABL, false>), grid, dim3(512), lds, s, g);
}
void launch_gemm_split_triples(const SplitGemmArgs& a, int ncomp, hipStream_t s, const Split3Launch& o) {
    if (a.K % SG_BK) throw HipError("gemm_split_triples: K must be a multiple of 32");
    if (!gemm_split_triples_fits(a.M, a.N, a.K, a.ldc)) throw HipError("gemm_split_triples: a component exceeds the 32-bit offset range");
    if (ncomp < 1 || a.ldc < a.N) throw HipError("gemm_split_triples: bad component count or output stride");
    static const bool walk_knob = tuning_env_int("IRSDE_SPLIT3_WALK", 1) != 0, drain_knob = tuning_env_int("IRSDE_SPLIT3_DRAIN", 0) != 0;
    const bool walk = o.walk == Split3Launch::RULE ? walk_knob : o.walk == Split3Launch::ON;
    const bool drain = o.drain == Split3Launch::RULE ? drain_knob : o.drain == Split3Launch::ON;
    if (drain && !walk) throw HipError("gemm_split_triples: the drain twin exists on the walk only");
    SplitGemmArgs g = a;
    g.nblk_n = (a.N + 127) / 128;
    g.n_inner = ncomp;   // an item = (component, row tile, column tile); n_inner carries the component count
    const long long units = (long long)((a.M + 255) / 256) * ncomp;
    long long per_xcd = 0;
    for (int x = 0; x < 8; ++x) per_xcd = std::max(per_xcd, (x + 1) * units / 8 - x * units / 8);
    long long blocks = 8 * per_xcd * g.nblk_n;   // one per item of the fullest XCD, times eight
    if (blocks >= 0x7fffffffll) throw HipError("gemm_split_triples: grid too large");
    if (walk) {   // (a cap below 8 would leave an XCD's items without a block: set_force_split3_blocks refuses it, and no gfx950 part has fewer CUs)
        const int forced = g_force_split3_blocks.load(std::memory_order_relaxed);
        blocks = std::min<long long>(blocks, std::max(8, forced > 0 ? forced : device_cu_count()));
    }
    const dim3 grid((unsigned)blocks);
    const size_t lds = (size_t)2 * (256 + 128) * 192;
    switch (o.abl) {
        case Split3Launch::FULL: launch_split3_abl<0>(walk, drain, grid, lds, s, g); break;
#ifdef IRSDE_PROBES
        case Split3Launch::NO_LOADS: launch_split3_abl<1>(walk, drain, grid, lds, s, g); break;
        case Split3Launch::NO_MFMA: launch_split3_abl<3>(walk, drain, grid, lds, s, g); break;
        case Split3Launch::NO_STORES: launch_split3_abl<4>(walk, drain, grid, lds, s, g); break;
#endif
        default: throw HipError("gemm_split_triples: the ablation twins are part of the PROBES build");
    }
    IRSDE_HIP_CHECK(hipGetLastError());
}

bool gemm_split3a_fits(const Split3aArgs& a, const char** why_not) {
    const char* why = nullptr;
    const unsigned long long lim = 0xffffffffull;
    const long long K = (long long)a.C0 + a.C1;
    if (a.M < 1 || a.N < 1) why = "empty";
    else if (a.C0 < 32 || a.C0 % SG_BK) why = "C0 not a multiple of 32";
    else if (a.C1 < 0 || a.C1 % SG_BK) why = "C1 not a multiple of 32";
    else if (a.pix0 < a.C0 || a.pix0 % 4 || (a.C1 && (a.pix1 < a.C1 || a.pix1 % 4)) || a.out_stride < a.N) why = "bad stride";
    // (the sources and the weights are addressed by 32-bit offsets from their bases; the output through a 64-bit base per wave and an offset inside its 32 rows)
    else if ((unsigned long long)a.M * a.pix0 * 4ull >= lim || (unsigned long long)a.M * a.pix1 * 4ull >= lim ||
             (unsigned long long)split3_comp_elems((size_t)a.N, (size_t)K) * 2ull >= lim || 32ull * a.out_stride * 4ull >= lim)
        why = "beyond the 32-bit offset range";
    if (why_not) *why_not = why;
    return !why;
}

int gemm_split3a_blocks(long long M, int N, int cus, bool walk) {
    const long long units = (M + 255) / 256;
    long long per_xcd = 0;
    for (int x = 0; x < 8; ++x) per_xcd = std::max(per_xcd, (x + 1) * units / 8 - x * units / 8);
    long long blocks = 8 * per_xcd * ((N + 127) / 128);   // one per item of the fullest XCD, times eight
    if (walk) blocks = std::min<long long>(blocks, std::max(8, cus));
    return blocks >= 0x7fffffffll ? -1 : (int)blocks;
}

Split3aArgs split3_1x1_args(const ConvParams& p, const unsigned short* w3) {
    Split3aArgs a;
    a.in0 = p.in0; a.C0 = p.C0; a.pix0 = p.pix0;
    a.in1 = p.C1 ? p.in1 : nullptr; a.C1 = p.C1; a.pix1 = p.C1 ? p.pix1 : 0;
    a.w3 = w3; a.bias = p.bias; a.out = p.out;
    a.M = p.B * p.Ho * p.Wo; a.N = p.Cout; a.out_stride = p.out_stride;
    return a;
}

// The rule (knob 1; measured per layer against the f32 kernels at B = 16 and B = 2 on 256 x 256 and at 16 x 512 x 512, and end to end; profiles/split3_1x1.md,
// sections 3 and 5):
//   * at least 128 output channels: the column tile is 128 wide, and the one narrower layer of the UNet (128 -> 64 at level 0, HBM-bound) is 5 - 19 % SLOWER;
//   * at least 1e10 executed FLOP.  Kernel for kernel every layer with Cout >= 128 is faster at all three batch shapes, but END TO END the B = 2 plan with its
//     layers adopted (6.4e9 FLOP each and less) ran 4 % slower than the parent (3.287 -> 3.151 img/s): the launches behind the adopted layers took longer than
//     the layers gained.  The floor sits above those layers; at B = 16 it keeps the eight res_conv (5.2e10) and the to_qkv from 1.3e10 on;
//   * 2048 rows and K = 128: the smallest values measured to win kernel for kernel.
static constexpr long long kSplit3x1MinRows = 2048;
static constexpr int kSplit3x1MinK = 128, kSplit3x1MinCout = 128;
static constexpr double kSplit3x1MinFlop = 1e10;
Split3x1Choice split3_1x1_choose(const ConvParams& p, bool exact_f32, int master, int knob, int cus) {
    Split3x1Choice c;
    const long long M = (long long)p.B * p.Ho * p.Wo;
    const char* why = nullptr;
    if (!exact_f32) why = "not the exact-fp32 engine";
    else if (master <= 0) why = "IRSDE_SPLIT3 = 0";
    else if (knob <= 0) why = "IRSDE_SPLIT3_1X1 = 0";
    else if (p.KH != 1 || p.KW != 1) why = "not a 1x1 convolution";
    else if (p.stride != 1) why = "stride";
    else if (p.in_shift) why = "in_shift";
    else if (p.pad_y || p.pad_x) why = "padding";
    else if (p.film) why = "film";
    else if (p.silu) why = "silu";
    else if (p.res) why = "res";
    else if (p.in_scale) why = "in_scale";
    else if (p.ch_scale) why = "ch_scale";
    else if (p.gate || p.gate_film) why = "gate";
    else if (p.shuffle) why = "shuffle";
    else if (p.ln_g) why = "ln_g";
    else if (p.in_bf16 || p.out_bf16 || p.in_f16 || p.out_f16) why = "16-bit storage";
    else if (p.w_bf || p.w_pair) why = "16-bit operands";
    else if (p.splits > 1) why = "split-K";
    else if (p.nz != 1) why = "batched";
    else if (M < 1 || M >= 0x7fffffffll) why = "empty";
    else gemm_split3a_fits(split3_1x1_args(p, nullptr), &why);
    if (!why && knob == 1) {
        const int K = p.C0 + p.C1;
        if (M < kSplit3x1MinRows) why = "rule: rows";
        else if (K < kSplit3x1MinK) why = "rule: K";
        else if (p.Cout < kSplit3x1MinCout) why = "rule: Cout";
        else if (2.0 * (double)M * K * p.Cout < kSplit3x1MinFlop) why = "rule: FLOP";
    }
    if (why) {
        c.why_not = why;
        return c;
    }
    c.adopt = true;
    c.grid = gemm_split3a_blocks(M, p.Cout, cus, true);
    c.lds = (int)kSplit3aLds;
    return c;
}

template <int ABL>
static void launch_split3a_abl(bool walk, bool drain, dim3 grid, hipStream_t s, const Split3aArgs& g) {
    if (drain) hipLaunchKernelGGL((gemm_split3a_kernel<ABL, true, true>), grid, dim3(512), kSplit3aLds, s, g);
    else if (walk) hipLaunchKernelGGL((gemm_split3a_kernel<ABL, true>), grid, dim3(512), kSplit3aLds, s, g);
    else hipLaunchKernelGGL((gemm_split3a_kernel<ABL, false>), grid, dim3(512), kSplit3aLds, s, g);
}
void launch_gemm_split3a(const Split3aArgs& a, hipStream_t s, const Split3Launch& o) {
    const char* why = nullptr;
    if (!gemm_split3a_fits(a, &why)) throw HipError(std::string("gemm_split3a: ") + why);
    if (!a.in0 || (a.C1 && !a.in1) || !a.w3 || !a.out) throw HipError("gemm_split3a: null operand");
    const bool walk = o.walk != Split3Launch::OFF, drain = o.drain == Split3Launch::ON;
    if (drain && !walk) throw HipError("gemm_split3a: the drain twin exists on the walk only");
    Split3aArgs g = a;
    g.nblk_n = (a.N + 127) / 128;
    const int forced = g_force_split3_blocks.load(std::memory_order_relaxed);
    const int blocks = gemm_split3a_blocks(a.M, a.N, forced > 0 ? forced : device_cu_count(), walk);
    if (blocks < 1) throw HipError("gemm_split3a: grid too large");
    const dim3 grid((unsigned)blocks);
    switch (o.abl) {
        case Split3Launch::FULL: launch_split3a_abl<0>(walk, drain, grid, s, g); break;
#ifdef IRSDE_PROBES
        case Split3Launch::NO_LOADS: launch_split3a_abl<1>(walk, drain, grid, s, g); break;
        case Split3Launch::NO_MFMA: launch_split3a_abl<3>(walk, drain, grid, s, g); break;
        case Split3Launch::NO_STORES: launch_split3a_abl<4>(walk, drain, grid, s, g); break;
#endif
        default: throw HipError("gemm_split3a: the ablation twins are part of the PROBES build");
    }
    IRSDE_HIP_CHECK(hipGetLastError());
}

void launch_split_triples(const float* in, unsigned short* out, int ncomp, size_t rows, int K, hipStream_t s) {
    if (K % 32 || ncomp < 1 || rows < 1) throw HipError("split_triples: K must be a multiple of 32");
    const size_t n = (size_t)ncomp * rows * (size_t)K;
    hipLaunchKernelGGL(split_triples_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, out, n, rows, K);
    IRSDE_HIP_CHECK(hipGetLastError());
}

void launch_split_pairs(const float* in, unsigned short* out, size_t rows, int K, hipStream_t s, bool f16, float scale) {
    if (K % 32) throw HipError("split_pairs: K must be a multiple of 32");
    const size_t n = rows * (size_t)K;
    if (f16) hipLaunchKernelGGL(split_pairs_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, out, n, K, scale);
    else hipLaunchKernelGGL(split_pairs_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, out, n, K, 1.0f);
    IRSDE_HIP_CHECK(hipGetLastError());
}

void launch_split_planes(const float* in, unsigned short* out, size_t n, size_t plane, int nplanes, hipStream_t s, bool f16, float scale) {
    const dim3 grid((unsigned)((n + 255) / 256));
    if (f16 && nplanes != 2) throw HipError("split_planes: fp16 pieces come in pairs");
    if (f16) hipLaunchKernelGGL((split_planes_kernel<2, true>), grid, dim3(256), 0, s, in, out, n, plane, scale);
    else if (nplanes == 2) hipLaunchKernelGGL((split_planes_kernel<2, false>), grid, dim3(256), 0, s, in, out, n, plane, 1.0f);
    else throw HipError("split_planes: 2 planes");
    IRSDE_HIP_CHECK(hipGetLastError());
}

}  // namespace irsde
