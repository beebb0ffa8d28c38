// LinearAttention of the IR-SDE score network for gfx950 (wave64) — module_util.py:150-178: the three-pass kernels on a q | k | v tensor and the
// two fused kernels that run PreNorm, the projections, the attention core, to_out and the residual without one (five projection modes, AttnMode).
// Built with -ffp-contract=off (Makefile, NOFMA), like kernels_misc.hip whose part this code was: contraction would change the kernels' bits.
// ---------------------------------------------------------------------------------------------
// LinearAttention.  qkv: [B][N][384] = q(4 heads x 32) | k | v.
//   q <- softmax over d (32, per pixel) * 32^-0.5 ; k <- softmax over N (per channel) ; v <- v / N
//   ctx[d][e] = sum_n k[d][n] v[e][n]          (32 x N) x (N x 32)   -> one 32x32 MFMA tile per head
//   out[e][n] = sum_d ctx[d][e] q[d][n]        (N x 32) x (32 x 32)
// Pass 1: per N-chunk, sum_n exp(k-m) and sum_n exp(k-m) v^T on v_mfma_f32_32x32x2_f32 with a running maximum m
//         (A[i=d][k=n] and B[k=n][j=e] are both 128-B coalesced rows straight from HBM; k and v are read once).
// Pass 2: combine chunks (exp(m_chunk - m) factors), fold 1/(S_d N) and the q scale into ctx.
// Pass 3: per 32-pixel tile: softmax(q) in registers (16 d per lane half + one permute), 16 MFMAs.
// ---------------------------------------------------------------------------------------------
#include "misc_shared.h"
#include <algorithm>
#include <string>
#include <type_traits>

namespace irsde {

namespace {

// 16-bit operand type of the fused attention kernels' projections: IEEE fp16 (the hi + lo pairs of IRSDE_FLAG_SPLIT_F16X2, IRSDE_FLAG_FP16) or
// bf16 (IRSDE_FLAG_BF16): the same 32x32x16 MFMA shape and fragment layout, fp32 accumulation
template <bool F16OP>
struct Mf16 {
    using x8 = bf16x8;
    using x4 = bf16x4;
    static __device__ __forceinline__ floatx16 mfma(x8 a, x8 b, floatx16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
template <>
struct Mf16<true> {
    using x8 = f16x8;
    using x4 = f16x4;
    static __device__ __forceinline__ floatx16 mfma(x8 a, x8 b, floatx16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};

// Pass 1+2 fused: one read of k and v.  Every wave keeps a running maximum of its pixels' k (per channel d) and rescales
// its context accumulator when the maximum grows (online softmax over N); the four waves and later the N-chunks are
// merged with exp(m_part - m_total) factors — the same sums as the two-pass form, without the separate max pass over k.
template <typename T>
__global__ __launch_bounds__(256) void attn_ctx_partial_kernel(const T* __restrict__ qkv, float* __restrict__ pmax,
                                                               float* __restrict__ pctx, float* __restrict__ psum,
                                                               const int N, const int chunk_len, const int nch) {
    __shared__ float red[4][1024 + 64];
    const int ch = blockIdx.x;
    const int bh = blockIdx.y;  // b*4 + head
    const int b = bh >> 2, head = bh & 3;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, h = lane >> 5;

    const int n0 = ch * chunk_len;
    const int n1 = min(N, n0 + chunk_len);
    const T* base = qkv + (size_t)b * N * kQkv + head * kDh + l31;
    floatx16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float ssum = 0.f;
    float mrun = -INFINITY;  // running max of k[d = l31] over this wave's pixels (same value in both lane halves)
    // wave w takes pixel pairs w, w+4, ...; lane half h takes pixel 2*pair + h
    constexpr int U = 8;  // 16 scalar loads (k, v of 8 pixel pairs) in flight per wave
    for (int pr = wave; 2 * pr < n1 - n0; pr += 4 * U) {
        float kx[U], vv[U];
        float mit = -INFINITY;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int n = n0 + 2 * (pr + 4 * u) + h;
            const bool ok = n < n1;
            const T* pp = base + (size_t)(ok ? n : n0) * kQkv;
            const float kl = ld1(pp + kHid), vl = ld1(pp + 2 * kHid);  // unconditional loads (clamped address), then select
            kx[u] = ok ? kl : -INFINITY;
            vv[u] = ok ? vl : 0.f;
            mit = fmaxf(mit, kx[u]);
        }
        mit = fmaxf(mit, __shfl_xor(mit, 32, 64));
        if (__any(mit > mrun)) {  // wave-uniform: after the first few iterations the maxima rarely move
            const float mnew = fmaxf(mrun, mit);  // finite: the first pixel pair of every wave-iteration exists
            const float alpha = expf(mrun - mnew);  // 0 on the first iteration (mrun = -inf)
            mrun = mnew;
            // the accumulator tile is ctx[d][e]: row d = (r&3) + 8(r>>2) + 4h needs the factor of channel d, which lives
            // in lane d of either half => fetch it with a lane read
            ssum *= alpha;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int d = (r & 3) + 8 * (r >> 2) + 4 * h;
                acc[r] *= __shfl(alpha, d, 64);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float e = expf(kx[u] - mrun);  // exp(-inf) = 0 for pixels past the chunk
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(e, vv[u], acc, 0, 0, 0);
            ssum += e;
        }
    }
    ssum += __shfl_xor(ssum, 32, 64);
    // merge the four waves: M = max_w m_w, scale wave w by exp(m_w - M)
    if (h == 0) red[wave][1024 + 32 + l31] = mrun;
    __syncthreads();
    float mblk = fmaxf(fmaxf(red[0][1024 + 32 + l31], red[1][1024 + 32 + l31]),
                       fmaxf(red[2][1024 + 32 + l31], red[3][1024 + 32 + l31]));
    const float wscale = mrun == -INFINITY ? 0.f : expf(mrun - mblk);  // a wave without pixels contributes nothing
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int d = (r & 3) + 8 * (r >> 2) + 4 * h;
        red[wave][d * 32 + l31] = acc[r] * __shfl(wscale, d, 64);
    }
    if (h == 0) red[wave][1024 + l31] = ssum * wscale;
    __syncthreads();
    float* oc = pctx + ((size_t)bh * nch + ch) * 1024;
    for (int i = threadIdx.x; i < 1024; i += 256) oc[i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
    if (threadIdx.x < 32) {
        const int i = 1024 + threadIdx.x;
        psum[((size_t)bh * nch + ch) * 32 + threadIdx.x] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
        pmax[((size_t)b * nch + ch) * kHid + head * kDh + threadIdx.x] = mblk;
    }
}

// LayerNorm of a row whose C/4 16-byte pieces sit in C/4 consecutive (aligned) lanes: two-pass mean / centred variance like
// layernorm_kernel (and torch.var / torch.mean), then * g.  C4 = C/4 is a power of two <= 64.
// Sum over an aligned group of W consecutive lanes (W a power of two <= 64), every lane of the group ends with the total.  r05: on the
// vector pipe only — DPP quad permutes / row mirrors inside a 16-lane row, v_permlane16_swap / v_permlane32_swap (gfx950) across rows —
// instead of __shfl_xor's ds_bpermute round trips (one LDS latency per butterfly step: 10 dependent steps per staged 16-byte piece put
// ~4.8k cycles of LDS latency into every 128-pixel tile of the fused attention kernels).  The mirror steps are valid because after the
// quad steps all lanes of a quad hold the same partial sum (and so on upwards); both operands of every add are the same two numbers in
// every lane of the group, so all lanes end with bit-identical totals.
// v_permlane16_swap / v_permlane32_swap (gfx950): rows 1, 3 (lanes 32 - 63) of the first operand change places with rows 0, 2 (lanes 0 - 31) of the second.
// With x in both operands the two results are [A A C C] / [B B D D] (resp. [lo lo] / [hi hi]): their sum (max) is the xor-16 (xor-32) butterfly step.
// Inline assembly on purpose (hipcc, ROCm 7.2; found by the parity tests, r05): through __builtin_amdgcn_permlane*_swap the optimiser folds the case
// "both operands hold the same value" into "both results = result 0" (also when the second operand is an identity DPP copy of the first), and
// `auto r = builtin(...); r[0], r[1]` reads element 0 twice even for different operands — either way the "sum" silently becomes 2 x one half.
// s_nop 1 = the two wait states the swap needs behind a VALU write of its operands (LLVM gfx950 hazard rule); the asm is opaque to the hazard recogniser.
struct SwapPair { float a, b; };
__device__ __forceinline__ SwapPair swap16(const float v) {
    SwapPair r{v, v};
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(r.a), "+v"(r.b));
    return r;
}
__device__ __forceinline__ SwapPair swap32(const float v) {
    SwapPair r{v, v};
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(r.a), "+v"(r.b));
    return r;
}
template <int W>
__device__ __forceinline__ float group_sum(float v) {
    static_assert(W >= 1 && W <= 64 && (W & (W - 1)) == 0, "group width must be a power of two <= 64");
    if constexpr (W >= 2) v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
    if constexpr (W >= 4) v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
    if constexpr (W >= 8) v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));  // row_half_mirror
    if constexpr (W >= 16) v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true)); // row_mirror
    if constexpr (W >= 32) {
        const SwapPair r = swap16(v);
        v = r.a + r.b;
    }
    if constexpr (W >= 64) {
        const SwapPair r = swap32(v);
        v = r.a + r.b;
    }
    return v;
}

// lane l and lane l ^ 32 combined (the two halves of a v_mfma_f32_32x32 accumulator column): v_permlane32_swap, no LDS round trip
__device__ __forceinline__ float half_sum(const float v) {
    const SwapPair r = swap32(v);
    return r.a + r.b;
}
__device__ __forceinline__ float half_max(const float v) {
    const SwapPair r = swap32(v);
    return fmaxf(r.a, r.b);
}

template <int C4>
__device__ __forceinline__ floatx4 ln_piece(floatx4 v, const floatx4 g, const float eps) {
    const float s = group_sum<C4>((v.x + v.y) + (v.z + v.w));
    const float mean = s * (1.0f / (float)(4 * C4));
    v -= mean;
    const float q = group_sum<C4>((v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w));
    // v_rsq_f32 (1 ulp) instead of 1 / sqrtf (v_sqrt + a full-precision division: ~15 vector instructions per piece on the pipe the f32 MFMAs share)
    const float rstd = __builtin_amdgcn_rsqf(q * (1.0f / (float)(4 * C4)) + eps);
    return v * rstd * g;
}

// the same for rows stored as bf16 (IRSDE_FLAG_BF16_ACT): a 16-byte piece holds 8 channels, a row = C8 = C/8 consecutive lanes (a power of two <= 32)
template <int C8>
__device__ __forceinline__ floatx8 ln_piece8(floatx8 v, const float* __restrict__ g8, const float eps) {
    const float s = group_sum<C8>(((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])));
    const float mean = s * (1.0f / (float)(8 * C8));
    v -= mean;
    const float q = group_sum<C8>(((v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3])) + ((v[4] * v[4] + v[5] * v[5]) + (v[6] * v[6] + v[7] * v[7])));
    const float rstd = __builtin_amdgcn_rsqf(q * (1.0f / (float)(8 * C8)) + eps);
    const floatx4 ga = *reinterpret_cast<const floatx4*>(g8), gb = *reinterpret_cast<const floatx4*>(g8 + 4);
    const floatx8 g = {ga.x, ga.y, ga.z, ga.w, gb.x, gb.y, gb.z, gb.w};
    return v * rstd * g;
}

// k, v projection + context in one kernel (fp32): the k and v thirds of to_qkv never reach HBM.
//   per 128-pixel tile of one image:  [k | v](128 px x 64) = xn(128 x C) . W_{k,v}^T   for each head (wave = head)
//   then straight from the accumulator registers: online softmax of k over the pixels and ctx[d][e] += exp(k - m)[px][d] v[px][e].
// The accumulator layout of v_mfma_f32_32x32x2_f32 (lane = column, registers = rows) is exactly the operand layout of the
// second product (A[i = d][k = pixel], B[k = pixel][j = e]: both indexed by the lane's column and a pixel pair picked by
// the register index and the lane half), so nothing is transposed or staged between the two GEMMs.
// xn tile in LDS ([128][C + 4]: odd number of 16-byte slots per row => conflict-free ds_read_b128), weight fragments
// straight from L2 (a wave's 64 weight rows x 8 k = two 16-byte loads per lane, one K step ahead).
// Output = the (max, sum, context) partials of attn_ctx_partial_kernel, merged by attn_ctx_finalize_kernel.
constexpr int kKvTile = 128;
// PAIR (r03, IRSDE_FLAG_SPLIT_F16X2): the k / v projection on v_mfma_f32_32x32x16_f16 with every operand as an fp16 hi + lo pair (three
// cross products per f32 product: fp32-equivalent, 3/16 of the f32-MFMA cycles): the staged tile is split while it is written to LDS
// (two planes of [128][C] fp16, rows of 2 C + 16 bytes), the weights come as two pre-split planes (wkv_pair: [2][256][C], scaled by
// the power of two that w_inv_scale undoes on the accumulators).  Everything after the projection (softmax, context) is unchanged f32.
// MODE (AttnMode, common.h; r05): 0 = F32, 1 = PairF16 (PAIR), 2 / 3 = Bf16 / Fp16, the 16-bit operand modes (IRSDE_FLAG_BF16 / IRSDE_FLAG_FP16; the reference is fp32 only): ONE bf16 / fp16 plane
// of the staged tile and of the weights (wkv_pair: [256][C], unscaled), one product per f32 product — with the projection at 1/16 of its f32
// cycles the kernel is bound by the tile it streams.  ABF (IRSDE_FLAG_BF16_ACT, MODE 2): xn is a bf16 tensor, pieces of 8 channels.
// MODE 4 (exact-fp32 engine, IRSDE_SPLIT3_ATTN): the k / v projection on v_mfma_f32_32x32x16_bf16 with every operand as THREE bf16 pieces (all 24 significand
// bits) and the six products of gemm_split3i_kernel (dropped terms <= 3 * 2^-27 |ab|): 6 MFMAs of 32 cycles instead of 8 of 64 per 16 channels.  The tile is split
// while it is staged (three planes, rows of 2 C + 16 bytes), the weights come as three unscaled planes in MFMA-fragment order (wkv_pair: 3 x [256][C], attn_frag3_index; bf16 has fp32's exponent
// range).  Softmax and the context product stay on the f32 pipe.  Sized to LDS: a 64-pixel tile (kKvTileTri) = 3 * 64 * (2 C + 16) bytes = 27.6 / 52.2 / 101.4 KB
// at C = 64 / 128 / 256, against the f32 kernel's 34.8 / 67.6 / 133 KB: LDS leaves room for 5 / 3 / 1 blocks per CU (f32: 4 / 2 / 1; launch_bounds caps both at
// two), so the serial phases of two blocks still overlap at C <= 128.  Cost of the smaller tile: a wave pulls its 64 weight rows x 3 planes = 384 C bytes from L2
// per 64 pixels (f32: 256 C per 128); with ~10 k cycles per tile and two waves per SIMD that is 4 * 384 C * 2 / 20 k = 9.8 / 19.7 / 39 B/clk per CU at
// C = 64 / 128 / 256 (C = 256, one block per CU: half of that) against the 27 - 35 B/clk the return path sustains (profiles/r06_notes.md, section 1).  That is
// the rate of USEFUL bytes: row-major planes return 128-byte lines of which a fragment load uses 32 bytes, four times the traffic — measured slower than the f32
// kernel (profiles/attn_split3.md, section 2) — hence the fragment order, in which a wave's load is one contiguous KB.
constexpr int kKvTileTri = 64;
template <int C, AttnMode MODE, bool ABF>
__global__ __launch_bounds__(256, 2) void attn_kv_ctx_kernel(const float* __restrict__ xn, const float* __restrict__ wkv,
                                                             float* __restrict__ pmax, float* __restrict__ pctx,
                                                             float* __restrict__ psum, const int N, const int chunk_len,
                                                             const int nch, const float* __restrict__ ln_g, const float ln_eps,
                                                             const unsigned short* __restrict__ wkv_pair = nullptr, const float w_inv_scale = 1.f) {
    extern __shared__ __attribute__((aligned(16))) float kv_smem[];
    constexpr bool PAIR = MODE == AttnMode::PairF16, TRI = MODE == AttnMode::Bf16x3, P16 = MODE != AttnMode::F32;
    using M16 = Mf16<MODE == AttnMode::PairF16 || MODE == AttnMode::Fp16>;
    static_assert(!ABF || MODE == AttnMode::Bf16, "bf16 activation storage goes with the bf16 operand mode");
    constexpr int TP = TRI ? kKvTileTri : kKvTile, NRT = TP / 32;   // pixels per tile, 32-pixel row tiles per tile
    constexpr int RB = 2 * C + 16;   // 16-bit modes: bytes per LDS row (an odd number of 16-byte slots)
    const int ch = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, head = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    constexpr int LDA = C + 4;
    const int n0 = ch * chunk_len;
    const int n1 = min(N, n0 + chunk_len);
    const float* wk = wkv + (size_t)(head * kDh + l31) * C + 4 * h;          // k rows of this head (to_qkv rows 128..255)
    const float* wv = wkv + (size_t)(kHid + head * kDh + l31) * C + 4 * h;   // v rows (256..383)
    constexpr int c4n = C >> 2;
    floatx16 ctx;
#pragma unroll
    for (int r = 0; r < 16; ++r) ctx[r] = 0.f;
    float ssum = 0.f, mrun = -INFINITY;
    for (int t0 = n0; t0 < n1; t0 += TP) {
        // stage the tile (rows past the chunk repeat its last pixel; they are masked below)
        auto stage_tile = [&](auto full_tag) {
            // r05: a full tile is one contiguous run of 128 * C floats (NHWC): element 4 i of it is piece i — no per-piece row / column / clamp arithmetic
            constexpr bool FULL = decltype(full_tag)::value;
            const float* tile = xn + ((size_t)b * N + t0) * C;
            // r05: 8 loads in flight before the first LDS write of a pass, passes unrolled (r02: a rolled loop of 4 — four exposed HBM round trips per
            // tile; the 144 accumulator registers it was fitted next to are not live while the tile is staged: they are zeroed behind the barrier)
            constexpr int NP = TP * c4n / 256;
            constexpr int NB = NP % 8 == 0 ? 8 : 4;
#pragma unroll
            for (int j0 = 0; j0 < NP; j0 += NB) {
                floatx4 st[NB];
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    int i = tid + 256 * (j0 + j), row, c4;
                    if constexpr (256 % c4n == 0) { row = tid / c4n + (256 / c4n) * (j0 + j); c4 = tid % c4n; }   // (no carry: tid < 256 — constants the compiler can fold into offsets)
                    else { row = i / c4n; c4 = i - row * c4n; }
                    if constexpr (FULL) st[j] = *reinterpret_cast<const floatx4*>(tile + 4 * i);
                    else st[j] = *reinterpret_cast<const floatx4*>(xn + ((size_t)b * N + min(t0 + row, n1 - 1)) * C + 4 * c4);
                }
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    int i = tid + 256 * (j0 + j), row, c4;
                    if constexpr (256 % c4n == 0) { row = tid / c4n + (256 / c4n) * (j0 + j); c4 = tid % c4n; }   // (no carry: tid < 256 — constants the compiler can fold into offsets)
                    else { row = i / c4n; c4 = i - row * c4n; }
                    // ln_g != nullptr: the input is the block's x and PreNorm's LayerNorm (module_util.py:82-90) runs here,
                    // on the staged pieces (power-of-two C only: a row = C/4 consecutive lanes)
                    if constexpr ((c4n & (c4n - 1)) == 0)
                        if (ln_g) st[j] = ln_piece<c4n>(st[j], *reinterpret_cast<const floatx4*>(ln_g + 4 * c4), ln_eps);
                    if constexpr (PAIR) {
                        const f16x4 hi = __builtin_convertvector(st[j], f16x4);
                        const f16x4 lo = __builtin_convertvector(st[j] - __builtin_convertvector(hi, floatx4), f16x4);
                        char* dst = reinterpret_cast<char*>(kv_smem) + row * RB + 8 * c4;
                        *reinterpret_cast<f16x4*>(dst) = hi;
                        *reinterpret_cast<f16x4*>(dst + TP * RB) = lo;
                    } else if constexpr (TRI) {   // three bf16 planes (the arithmetic of split_triples_kernel: every residual is exact in f32)
                        const bf16x4 p0 = __builtin_convertvector(st[j], bf16x4);
                        const floatx4 r1 = st[j] - __builtin_convertvector(p0, floatx4);
                        const bf16x4 p1 = __builtin_convertvector(r1, bf16x4);
                        const bf16x4 p2 = __builtin_convertvector(r1 - __builtin_convertvector(p1, floatx4), bf16x4);
                        char* dst = reinterpret_cast<char*>(kv_smem) + row * RB + 8 * c4;
                        *reinterpret_cast<bf16x4*>(dst) = p0;
                        *reinterpret_cast<bf16x4*>(dst + TP * RB) = p1;
                        *reinterpret_cast<bf16x4*>(dst + 2 * TP * RB) = p2;
                    } else if constexpr (P16) {   // one plane, RNE
                        *reinterpret_cast<typename M16::x4*>(reinterpret_cast<char*>(kv_smem) + row * RB + 8 * c4) = __builtin_convertvector(st[j], typename M16::x4);
                    } else {
                        *reinterpret_cast<floatx4*>(kv_smem + row * LDA + 4 * c4) = st[j];
                    }
                }
            }
        };
        // ABF: the tile is 128 * C bf16 (one contiguous run), 16-byte pieces of 8 channels, a row = C / 8 consecutive lanes
        auto stage_tile_bf = [&](auto full_tag) {
            constexpr bool FULL = decltype(full_tag)::value;
            constexpr int c8n = C >> 3;
            const char* xb = reinterpret_cast<const char*>(xn);
            const char* tile = xb + ((size_t)b * N + t0) * C * 2;
            constexpr int NP = TP * c8n / 256;
            constexpr int NB = NP % 8 == 0 ? 8 : 4;
            static_assert(256 % c8n == 0 && NP % NB == 0, "piece / thread mapping");
#pragma unroll
            for (int j0 = 0; j0 < NP; j0 += NB) {
                bf16x8 st[NB];
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    const int i = tid + 256 * (j0 + j), row = tid / c8n + (256 / c8n) * (j0 + j), c8 = tid % c8n;
                    if constexpr (FULL) st[j] = *reinterpret_cast<const bf16x8*>(tile + 16 * (size_t)i);
                    else st[j] = *reinterpret_cast<const bf16x8*>(xb + (((size_t)b * N + min(t0 + row, n1 - 1)) * C + 8 * c8) * 2);
                }
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    const int row = tid / c8n + (256 / c8n) * (j0 + j), c8 = tid % c8n;
                    if (ln_g) st[j] = __builtin_convertvector(ln_piece8<c8n>(__builtin_convertvector(st[j], floatx8), ln_g + 8 * c8, ln_eps), bf16x8);
                    *reinterpret_cast<bf16x8*>(reinterpret_cast<char*>(kv_smem) + row * RB + 16 * c8) = st[j];
                }
            }
        };
        // TRI: the weight fragments (three planes of the lane's k and v row) one K step ahead in two register slots; the first step's go out in front of the
        // staging, which hides their L2 round trip (they do not depend on the tile)
        [[maybe_unused]] bf16x8 wk3[2][3], wv3[2][3];   // [slot][piece]
        [[maybe_unused]] const char* wkp3 = TRI ? reinterpret_cast<const char*>(wkv_pair) + ((size_t)head * (C / 16) * 64 + 32 * h + l31) * 16 : nullptr;          // row tile = head
        [[maybe_unused]] const char* wvp3 = TRI ? reinterpret_cast<const char*>(wkv_pair) + ((size_t)(kHeads + head) * (C / 16) * 64 + 32 * h + l31) * 16 : nullptr;   // row tile = 4 + head
        constexpr size_t WPL3 = (size_t)2 * kHid * C * 2;   // bytes between two weight planes (wkv_pair: three planes of [256][C] in fragment order, attn_frag3_index: a K step = 1 KB)
        if constexpr (TRI) {
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                wk3[0][p] = *reinterpret_cast<const bf16x8*>(wkp3 + p * WPL3);
                wv3[0][p] = *reinterpret_cast<const bf16x8*>(wvp3 + p * WPL3);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (ABF) {
            if (t0 + TP <= n1) stage_tile_bf(std::true_type{}); else stage_tile_bf(std::false_type{});
        } else {
            if (t0 + TP <= n1) stage_tile(std::true_type{}); else stage_tile(std::false_type{});
        }
        __syncthreads();
        floatx16 ak[NRT], av[NRT];
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r) { ak[rt][r] = 0.f; av[rt][r] = 0.f; }
        if constexpr (PAIR) {
            // K steps of 16: lane (row l31, half h) holds k = 16 ks + 8 h .. + 7 of the A rows (pixels) and of its weight row
            const char* arow = reinterpret_cast<const char*>(kv_smem) + l31 * RB + 16 * h;
            const char* wkp = reinterpret_cast<const char*>(wkv_pair) + ((size_t)(head * kDh + l31) * C + 8 * h) * 2;
            const char* wvp = reinterpret_cast<const char*>(wkv_pair) + ((size_t)(kHid + head * kDh + l31) * C + 8 * h) * 2;
            constexpr size_t WPL = (size_t)2 * kHid * C * 2;   // bytes between the hi and the lo weight plane
            constexpr int NK16 = C / 16;
            f16x8 wk2[2][2], wv2[2][2];   // [slot][plane], one K step ahead
            wk2[0][0] = *reinterpret_cast<const f16x8*>(wkp);
            wk2[0][1] = *reinterpret_cast<const f16x8*>(wkp + WPL);
            wv2[0][0] = *reinterpret_cast<const f16x8*>(wvp);
            wv2[0][1] = *reinterpret_cast<const f16x8*>(wvp + WPL);
            auto kstep = [&](const int ks) {
                const int cur = ks & 1, nxt = cur ^ 1;
                const int kp = (ks + 1 < NK16 ? ks + 1 : ks) * 32;
                wk2[nxt][0] = *reinterpret_cast<const f16x8*>(wkp + kp);
                wk2[nxt][1] = *reinterpret_cast<const f16x8*>(wkp + WPL + kp);
                wv2[nxt][0] = *reinterpret_cast<const f16x8*>(wvp + kp);
                wv2[nxt][1] = *reinterpret_cast<const f16x8*>(wvp + WPL + kp);
#pragma unroll
                for (int rt = 0; rt < NRT; ++rt) {
                    const f16x8 ah = *reinterpret_cast<const f16x8*>(arow + rt * 32 * RB + 32 * ks);
                    const f16x8 al = *reinterpret_cast<const f16x8*>(arow + TP * RB + rt * 32 * RB + 32 * ks);
                    ak[rt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, wk2[cur][1], ak[rt], 0, 0, 0);
                    av[rt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, wv2[cur][1], av[rt], 0, 0, 0);
                    ak[rt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, wk2[cur][0], ak[rt], 0, 0, 0);
                    av[rt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, wv2[cur][0], av[rt], 0, 0, 0);
                    ak[rt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, wk2[cur][0], ak[rt], 0, 0, 0);
                    av[rt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, wv2[cur][0], av[rt], 0, 0, 0);
                }
            };
            // C >= 128: unrolled by two (the register ping-pong needs an even factor) — the full unroll of 16 (8) steps spilled 236 (72) VGPRs;
            // the 4-step loop of C = 64 stays fully unrolled (measured 9 % slower at 2)
            if constexpr (C > 64) {
#pragma unroll 2
                for (int ks = 0; ks < NK16; ++ks) kstep(ks);
            } else {
#pragma unroll
                for (int ks = 0; ks < NK16; ++ks) kstep(ks);
            }
#pragma unroll
            for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
                for (int r = 0; r < 16; ++r) { ak[rt][r] *= w_inv_scale; av[rt][r] *= w_inv_scale; }
        } else if constexpr (TRI) {
            // three bf16 pieces per operand, the six products of gemm_split3i_kernel in its order (a0 b2, a1 b1, a2 b0, a0 b1, a1 b0, a0 b0: smallest first),
            // K steps of 16: lane (row l31, half h) holds k = 16 ks + 8 h .. + 7 of its pixel rows (three LDS planes) and of its weight rows
            const char* arow = reinterpret_cast<const char*>(kv_smem) + l31 * RB + 16 * h;
            constexpr int NK16 = C / 16;
            auto kstep = [&](const int ks) {
                const int cur = ks & 1, nxt = cur ^ 1;
                const int kp = (ks + 1 < NK16 ? ks + 1 : ks) * 1024;
#pragma unroll
                for (int p = 0; p < 3; ++p) {
                    wk3[nxt][p] = *reinterpret_cast<const bf16x8*>(wkp3 + p * WPL3 + kp);
                    wv3[nxt][p] = *reinterpret_cast<const bf16x8*>(wvp3 + p * WPL3 + kp);
                }
#pragma unroll
                for (int rt = 0; rt < NRT; ++rt) {
                    const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(arow + rt * 32 * RB + 32 * ks);
                    const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(arow + TP * RB + rt * 32 * RB + 32 * ks);
                    const bf16x8 a2 = *reinterpret_cast<const bf16x8*>(arow + 2 * TP * RB + rt * 32 * RB + 32 * ks);
                    ak[rt] = M16::mfma(a0, wk3[cur][2], ak[rt]);
                    av[rt] = M16::mfma(a0, wv3[cur][2], av[rt]);
                    ak[rt] = M16::mfma(a1, wk3[cur][1], ak[rt]);
                    av[rt] = M16::mfma(a1, wv3[cur][1], av[rt]);
                    ak[rt] = M16::mfma(a2, wk3[cur][0], ak[rt]);
                    av[rt] = M16::mfma(a2, wv3[cur][0], av[rt]);
                    ak[rt] = M16::mfma(a0, wk3[cur][1], ak[rt]);
                    av[rt] = M16::mfma(a0, wv3[cur][1], av[rt]);
                    ak[rt] = M16::mfma(a1, wk3[cur][0], ak[rt]);
                    av[rt] = M16::mfma(a1, wv3[cur][0], av[rt]);
                    ak[rt] = M16::mfma(a0, wk3[cur][0], ak[rt]);
                    av[rt] = M16::mfma(a0, wv3[cur][0], av[rt]);
                }
            };
            if constexpr (C > 64) {   // (as PAIR: the register ping-pong needs an even factor)
#pragma unroll 2
                for (int ks = 0; ks < NK16; ++ks) kstep(ks);
            } else {
#pragma unroll
                for (int ks = 0; ks < NK16; ++ks) kstep(ks);
            }
        } else if constexpr (P16) {
            // one 16-bit plane: K steps of 16, lane (row l31, half h) holds k = 16 ks + 8 h .. + 7 of its pixel rows and of its weight rows
            using x8 = typename M16::x8;
            const char* arow = reinterpret_cast<const char*>(kv_smem) + l31 * RB + 16 * h;
            const char* wkp = reinterpret_cast<const char*>(wkv_pair) + ((size_t)(head * kDh + l31) * C + 8 * h) * 2;
            const char* wvp = reinterpret_cast<const char*>(wkv_pair) + ((size_t)(kHid + head * kDh + l31) * C + 8 * h) * 2;
            constexpr int NK16 = C / 16;
            x8 wk1[2], wv1[2];   // one K step ahead
            wk1[0] = *reinterpret_cast<const x8*>(wkp);
            wv1[0] = *reinterpret_cast<const x8*>(wvp);
#pragma unroll
            for (int ks = 0; ks < NK16; ++ks) {
                const int cur = ks & 1, nxt = cur ^ 1;
                const int kp = (ks + 1 < NK16 ? ks + 1 : ks) * 32;
                wk1[nxt] = *reinterpret_cast<const x8*>(wkp + kp);
                wv1[nxt] = *reinterpret_cast<const x8*>(wvp + kp);
#pragma unroll
                for (int rt = 0; rt < NRT; ++rt) {
                    const x8 a = *reinterpret_cast<const x8*>(arow + rt * 32 * RB + 32 * ks);
                    ak[rt] = M16::mfma(a, wk1[cur], ak[rt]);
                    av[rt] = M16::mfma(a, wv1[cur], av[rt]);
                }
            }
        } else {
            const float* arow = kv_smem + l31 * LDA + 4 * h;
            // weight fragments (from L2) one K step = 32 MFMAs (2048 cycles) ahead of their use: two register slots, K loop
            // unrolled by two only (a full unroll of up to 32 steps x 32 MFMAs spills)
            constexpr int NK = C / 8;
            static_assert(NK % 2 == 0, "C must be a multiple of 16");
            floatx4 wkr[2], wvr[2];
            wkr[0] = *reinterpret_cast<const floatx4*>(wk);
            wvr[0] = *reinterpret_cast<const floatx4*>(wv);
#pragma unroll 1
            for (int ks0 = 0; ks0 < NK; ks0 += 2)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int ks = ks0 + u;
                const int k8 = 8 * ks;
                {
                    const int kp = ks + 1 < NK ? k8 + 8 : k8;  // past the end: a harmless reload
                    wkr[u ^ 1] = *reinterpret_cast<const floatx4*>(wk + kp);
                    wvr[u ^ 1] = *reinterpret_cast<const floatx4*>(wv + kp);
                }
                __builtin_amdgcn_sched_barrier(0);  // keep the prefetch in front of this step's MFMAs
                const floatx4 bk = wkr[u], bv = wvr[u];
#pragma unroll
                for (int rt = 0; rt < NRT; ++rt) {
                    const floatx4 a = *reinterpret_cast<const floatx4*>(arow + rt * 32 * LDA + k8);
                    ak[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bk.x, ak[rt], 0, 0, 0);
                    av[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bv.x, av[rt], 0, 0, 0);
                    ak[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bk.y, ak[rt], 0, 0, 0);
                    av[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bv.y, av[rt], 0, 0, 0);
                    ak[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bk.z, ak[rt], 0, 0, 0);
                    av[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bv.z, av[rt], 0, 0, 0);
                    ak[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bk.w, ak[rt], 0, 0, 0);
                    av[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bv.w, av[rt], 0, 0, 0);
                }
            }
        }
        // accumulator register r of row tile rt: pixel t0 + 32 rt + (r&3) + 8 (r>>2) + 4h, column d (k) / e (v) = l31
        float mit = -INFINITY;
        if (t0 + TP > n1) {   // (uniform) only the last tile of a chunk has pixels to mask: 128 compares + 256 selects per lane otherwise
#pragma unroll
            for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int n = t0 + 32 * rt + (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (n >= n1) { ak[rt][r] = -INFINITY; av[rt][r] = 0.f; }
                }
        }
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r) mit = fmaxf(mit, ak[rt][r]);
        mit = half_max(mit);
        if (__any(mit > mrun)) {  // wave-uniform; the tile's first pixel exists, so mnew is finite
            const float mnew = fmaxf(mrun, mit);
            const float alpha = expf(mrun - mnew);  // 0 on the first tile (mrun = -inf)
            mrun = mnew;
            ssum *= alpha;
            // context row d = (r&3) + 8(r>>2) + 4h needs the factor of channel d, which lives in lane d of either half
#pragma unroll
            for (int r = 0; r < 16; ++r) ctx[r] *= __shfl(alpha, (r & 3) + 8 * (r >> 2) + 4 * h, 64);
        }
        // exp(k - m) for the whole tile FIRST (one fma + v_exp_f32 per element, in place), then the 64 MFMAs back to back:
        // a vector instruction between two f32 MFMAs costs its own time plus ~16 cycles (tools/probe/mfma_valu_samewave.hip),
        // and expf() in front of every MFMA (~17 instructions) made each of them cost ~150 cycles instead of 64.  The common
        // factor 2^(-m log2e) carries one rounding of m log2e; it is the same for every pixel of channel d and cancels
        // against ssum.  exp2(-inf) = 0 for the masked pixels.
        {
            const float ml = mrun * 1.44269504088896341f;
#pragma unroll
            for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    ak[rt][r] = __builtin_amdgcn_exp2f(__builtin_fmaf(ak[rt][r], 1.44269504088896341f, -ml));
                    ssum += ak[rt][r];
                }
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (MODE == AttnMode::Bf16 || MODE == AttnMode::Fp16) {
            // 16-bit operand modes: the context product on the 16-bit MFMA too — exp(k - m) in [0, 1] and v rounded once (RNE), fp32 accumulation.  A K step
            // of 16 pixels takes the lane's registers 8 s .. 8 s + 7 of a row tile for A (its column d) and B (its column e) alike: the same pixel
            // order in both operands, 8 MFMAs of 8 passes instead of 64 of 16.  (ssum stays the fp32 sum of the unrounded exponentials.)
            using x8 = typename M16::x8;
#pragma unroll
            for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
                for (int sh = 0; sh < 2; ++sh) {
                    const floatx8 ka = {ak[rt][8 * sh], ak[rt][8 * sh + 1], ak[rt][8 * sh + 2], ak[rt][8 * sh + 3],
                                        ak[rt][8 * sh + 4], ak[rt][8 * sh + 5], ak[rt][8 * sh + 6], ak[rt][8 * sh + 7]};
                    const floatx8 va = {av[rt][8 * sh], av[rt][8 * sh + 1], av[rt][8 * sh + 2], av[rt][8 * sh + 3],
                                        av[rt][8 * sh + 4], av[rt][8 * sh + 5], av[rt][8 * sh + 6], av[rt][8 * sh + 7]};
                    ctx = M16::mfma(__builtin_convertvector(ka, x8), __builtin_convertvector(va, x8), ctx);
                }
        } else {
#pragma unroll
            for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
                for (int r = 0; r < 16; ++r) ctx = __builtin_amdgcn_mfma_f32_32x32x2f32(ak[rt][r], av[rt][r], ctx, 0, 0, 0);
        }
        __syncthreads();  // every wave is done with the tile in LDS
    }
    ssum = half_sum(ssum);
    const int bh = b * kHeads + head;
    float* oc = pctx + ((size_t)bh * nch + ch) * 1024;
#pragma unroll
    for (int r = 0; r < 16; ++r) oc[((r & 3) + 8 * (r >> 2) + 4 * h) * 32 + l31] = ctx[r];
    if (h == 0) {
        psum[((size_t)bh * nch + ch) * 32 + l31] = ssum;
        pmax[((size_t)b * nch + ch) * kHid + head * kDh + l31] = mrun;
    }
}

// Merge of the chunk partials: ctx[d][e] = sum_c pctx_c[d][e] e^{m_c[d] - m[d]} / sum_c psum_c[d] e^{m_c[d] - m[d]} / N * scale.
// grid (B * heads, 4): block = 8 context rows d of one (image, head); 1024 threads = 256 elements x 4 chunk slices (r05: one block of 1024
// threads per (image, head) walked all chunks serially — at the small batches of the strong-scaling shards (B = 2: 256 chunks per image, 8 blocks
// on the chip) that took longer than the k / v kernel it follows).  The slices are combined in fixed order: deterministic.
__global__ __launch_bounds__(1024) void attn_ctx_finalize_kernel(const float* __restrict__ pctx,
                                                                 const float* __restrict__ psum,
                                                                 const float* __restrict__ pmax,
                                                                 float* __restrict__ ctx, const int nch,
                                                                 const float inv_n, const float scale) {
    __shared__ float sm[4][8];
    __shared__ float ss[4][256];
    __shared__ float sz[4][8];
    const int bh = blockIdx.x, dq = blockIdx.y;
    const int b = bh >> 2, head = bh & 3;
    const int el = threadIdx.x & 255, sl = threadIdx.x >> 8;
    const int dl = el >> 5, e = el & 31, d = 8 * dq + dl;
    const float* pm = pmax + (size_t)b * nch * kHid + head * kDh + d;
    float mx = -INFINITY;
    for (int c = sl; c < nch; c += 4) mx = fmaxf(mx, pm[(size_t)c * kHid]);
    if (e == 0) sm[sl][dl] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(sm[0][dl], sm[1][dl]), fmaxf(sm[2][dl], sm[3][dl]));
    const float* pc = pctx + (size_t)bh * nch * 1024 + d * 32 + e;
    const float* ps = psum + (size_t)bh * nch * 32 + d;
    float s = 0.f, z = 0.f;
#pragma unroll 4
    for (int c = sl; c < nch; c += 4) {
        const float w = expf(pm[(size_t)c * kHid] - mx);
        s += pc[(size_t)c * 1024] * w;
        z += ps[(size_t)c * 32] * w;
    }
    ss[sl][el] = s;
    if (e == 0) sz[sl][dl] = z;
    __syncthreads();
    if (sl == 0) {
        const float st = (ss[0][el] + ss[1][el]) + (ss[2][el] + ss[3][el]);
        const float zt = (sz[0][dl] + sz[1][dl]) + (sz[2][dl] + sz[3][dl]);
        ctx[(size_t)bh * 1024 + d * 32 + e] = st / zt * inv_n * scale;
    }
}

constexpr int kOutTilesPerBlock = 8;  // 256 pixels per block

template <typename T>
__global__ __launch_bounds__(256) void attn_out_kernel(const T* __restrict__ qkv, const float* __restrict__ ctx,
                                                       T* __restrict__ out, const int N, const int qstride) {
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63, head = threadIdx.x >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    // B operand: ctx[d = 16h + s][e = l31]
    float cb[16];
    const float* cp = ctx + ((size_t)(b * kHeads + head)) * 1024 + (16 * h) * 32 + l31;
#pragma unroll
    for (int s = 0; s < 16; ++s) cb[s] = cp[s * 32];

    // the q rows of tile t+1 are loaded before the softmax / MFMAs of tile t (one tile of loads always in flight)
    auto load_q = [&](int t, float* dst) {
        const int nb = (blockIdx.x * kOutTilesPerBlock + t) * 32;
        const int nn = nb + l31;
        const T* qp = qkv + ((size_t)b * N + (nn < N ? nn : (nb < N ? nb : 0))) * qstride + head * kDh + 16 * h;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const float4 t4 = ld4(qp + 4 * v);
            dst[4 * v + 0] = t4.x; dst[4 * v + 1] = t4.y; dst[4 * v + 2] = t4.z; dst[4 * v + 3] = t4.w;
        }
    };
    float qn[16];
    load_q(0, qn);
    for (int t = 0; t < kOutTilesPerBlock; ++t) {
        const int nbase = (blockIdx.x * kOutTilesPerBlock + t) * 32;
        if (nbase >= N) break;
        float q[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) q[s] = qn[s];
        if (t + 1 < kOutTilesPerBlock) load_q(t + 1, qn);
        float m = q[0];
#pragma unroll
        for (int s = 1; s < 16; ++s) m = fmaxf(m, q[s]);
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        float z = 0.f;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            q[s] = expf(q[s] - m);
            z += q[s];
        }
        z += __shfl_xor(z, 32, 64);
        const float iz = 1.0f / z;
        floatx16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(q[s] * iz, cb[s], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            const int nn = nbase + row;
            if (nn < N) st1(out + ((size_t)b * N + nn) * kHid + head * kDh + l31, acc[r]);
        }
    }
}

// q projection + softmax over d + context product + to_out + bias + LayerNorm + residual in one kernel (fp32, C = 64 / 128):
// neither q nor the attention output nor the to_out result reach HBM — the second half of the fused LinearAttention block
// (module_util.py:163-178: q.softmax(dim=-2) * scale, einsum with the context, to_out = Conv2d + LayerNorm, Residual).
// One block = 128 pixels of one image, 4 waves:
//   A  xn tile -> LDS Xs[128][C+4]
//   B  wave = head: Q^T[d][px] = Wq_h . xn^T   (A operand = weight rows straight from L2, B operand = Xs rows): 4 pixel tiles
//   C  softmax over d in registers: the lane's 16 rows + the other lane half (the 1/sqrt(32) scale is folded into ctx)
//   D  out^T[e][px] = ctx^T . softmax(q): A = 16 preloaded context registers, B = the lane's own q registers (the accumulator
//      layout of B is the operand layout of D: no transposition)
//   E  out tile -> LDS Os[128][128+4] (row = pixel, column = head*32 + e)
//   F  wave = 32-pixel tile: y^T[c][px] = Wout . out^T  (A = to_out rows from L2, B = Os rows), + bias
//   G  LayerNorm over c in registers (C/32 x 16 values + the other lane half), * g, -> LDS (the wave's own rows), then
//      coalesced 16-byte passes: + x (residual), store y.
// PAIR (r03, IRSDE_FLAG_SPLIT_F16X2): the two projections (B: q, F: to_out) on v_mfma_f32_32x32x16_f16 with fp16 hi + lo operand
// pairs (three cross products per f32 product): the xn tile and the attention-output tile are written to LDS as two fp16 planes
// (rows of 2 C + 16 resp. 272 bytes), the weights come as pre-split planes (wq_pair [2][128][C], wout_pair [2][C][128], scaled by powers
// of two that wq_inv / wout_inv undo on the accumulators).  Softmax, the context product, LayerNorm and the residual stay f32.
// MODE 2 / 3 (r05; IRSDE_FLAG_BF16 / IRSDE_FLAG_FP16): one bf16 / fp16 plane per operand (wq_pair [128][C], wout_pair [C][128], unscaled), one product.
// ABF (IRSDE_FLAG_BF16_ACT, MODE 2): xn / xres / y are bf16 tensors (pieces of 8 channels); the arithmetic between them is the same fp32.
// MODE 4 (exact-fp32 engine, IRSDE_SPLIT3_ATTN): the two projections on three bf16 pieces per operand and six products (see attn_kv_ctx_kernel), the xn tile and the
// attention-output tile split while they are written to LDS, weights as three unscaled planes in MFMA-fragment order (wq_pair 3 x [128][C], wout_pair 3 x [C][128]).  Sized to LDS: a
// 64-pixel tile (kQoTileTri).  Region = max(xn planes 3 * 64 * (2 C + 16), output planes 3 * 64 * 272 = 52.2 KB, normalised rows 64 * (max(C, 128) + 4) * 4) + 1 KB of
// LayerNorm partial sums = 53.2 / 53.2 / 102.4 KB at C = 64 / 128 / 256 (f32: 67.6 / 67.6 / 133 KB): two blocks per CU at C <= 128 (launch_bounds; LDS would
// hold three), one at C = 256, as the f32 kernel.  Waves: phases B - E wave = head over two 32-pixel tiles; phase F wave = (pixel tile, half of the output channels).  Weight
// fragments from L2 per block and tile: 3 * 2 * (128 C + C 128) = 1536 C bytes (f32, per 128 pixels: 1024 C) — at ~12 k cycles per tile and two waves per SIMD
// 2 * 1536 C / 24 k = 8 / 16 / 33 B/clk per CU at C = 64 / 128 / 256 (C = 256 with one block per CU: half).
constexpr int kQoTileTri = 64;
constexpr size_t qo_tri_main_bytes(const int C) {
    const size_t px = (size_t)3 * kQoTileTri * (2 * C + 16), po = (size_t)3 * kQoTileTri * (2 * kHid + 16), ys = (size_t)kQoTileTri * ((C > kHid ? C : kHid) + 4) * 4;
    return px > po ? (px > ys ? px : ys) : (po > ys ? po : ys);
}
template <int C, AttnMode MODE, bool ABF>
__global__ __launch_bounds__(256, 2) void attn_q_out_fused_kernel(const float* __restrict__ xn, const float* __restrict__ xres,
                                                               const float* __restrict__ wq, const float* __restrict__ ctx,
                                                               const float* __restrict__ wout, const float* __restrict__ bias,
                                                               const float* __restrict__ g2, float* __restrict__ y, const int N,
                                                               const float eps, const float* __restrict__ ln_g,
                                                               const unsigned short* __restrict__ wq_pair = nullptr,
                                                               const unsigned short* __restrict__ wout_pair = nullptr, const float wq_inv = 1.f,
                                                               const float wout_inv = 1.f) {
    constexpr bool PAIR = MODE == AttnMode::PairF16, TRI = MODE == AttnMode::Bf16x3, P16 = MODE != AttnMode::F32;
    constexpr int TP = TRI ? kQoTileTri : 128, LDA = C + 4, LDO = kHid + 4, RT = C / 32;
    constexpr int NCT = TP / 32, SL = TP / 4;   // 32-pixel tiles per block; rows of the slab a wave stages (phase A) and stores (phase G)
    using M16 = Mf16<MODE == AttnMode::PairF16 || MODE == AttnMode::Fp16>;
    static_assert(!ABF || MODE == AttnMode::Bf16, "bf16 activation storage goes with the bf16 operand mode");
    constexpr int RBX = 2 * C + 16, RBO = 2 * kHid + 16;   // 16-bit modes: bytes per row of the xn / attention-output planes
    constexpr int LDY = C > kHid ? C + 4 : LDO;  // row stride of the normalised rows (phase G): they must not overlap the next wave's rows
    extern __shared__ __attribute__((aligned(16))) float qo_smem[];
    // one LDS region (67.6 KB -> two blocks per CU, whose phases overlap): the xn tile (phases A, B), then — behind a barrier —
    // the attention output tile (E, F), then, wave-locally, the normalised rows (G)
    float* Xs = qo_smem;  // [128][C+4]
    float* Os = qo_smem;  // [128][132]
    const int b = blockIdx.y, t0 = blockIdx.x * TP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const size_t img = (size_t)b * N;

    // ---- A: stage the xn tile (rows past N repeat the last pixel; their results are never stored)
    constexpr int C4 = C / 4;
    const bool full_tile = t0 + TP <= N;   // uniform; a full tile is one contiguous run of 128 * C floats (r05: no per-piece index arithmetic)
    // r05: wave w stages ITS OWN 32-row slab of the tile (pieces i = lane + 64 j of the slab: the same pieces it adds back and stores in phase G), so when
    // the residual IS the staged tensor (xres == xn: the PreNorm-fused plan) the raw pieces stay in registers across the block (C <= 128: 32 / 64
    // registers of the 256 a wave has) and phase G neither re-reads the tile nor waits for it
    constexpr int NQ = SL * C4 / 64;
    constexpr bool KEEP = !PAIR && !ABF && C <= 128;
    floatx4 xkeep[KEEP ? NQ : 1];
    // ABF: the wave's slab is 32 * C bf16; pieces of 8 channels, a row = C8 consecutive lanes; the raw pieces stay in registers (C / 4 of them) for C <= 128
    constexpr int C8 = C / 8, NQ8 = 32 * C8 / 64;
    constexpr bool KEEP8 = ABF && C <= 128;
    const bool keep_res = (KEEP || KEEP8) && full_tile && xres == xn;
    bf16x8 xkeep8[KEEP8 ? NQ8 : 1];
    auto stage_tile = [&](auto full_tag) {
        constexpr bool FULL = decltype(full_tag)::value;
        const float* slab_in = xn + (img + t0 + wave * SL) * C;
        // 8 loads in flight before the first LDS write of a pass (a rolled loop waits for every load in turn)
        constexpr int NB = NQ < 8 ? NQ : 8;
#pragma unroll
        for (int j0 = 0; j0 < NQ; j0 += NB) {
            floatx4 st[NB];
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const int i = lane + 64 * (j0 + j), row = wave * SL + lane / C4 + (64 / C4) * (j0 + j), c4 = lane % C4;   // (C4 divides 64)
                if constexpr (FULL) st[j] = *reinterpret_cast<const floatx4*>(slab_in + 4 * i);
                else st[j] = *reinterpret_cast<const floatx4*>(xn + (img + min(t0 + row, N - 1)) * C + 4 * c4);
                if constexpr (FULL && KEEP) xkeep[j0 + j] = st[j];
            }
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const int row = wave * SL + lane / C4 + (64 / C4) * (j0 + j), c4 = lane % C4;
                // ln_g != nullptr: xn == the block's x and PreNorm's LayerNorm runs here on the staged pieces
                if (ln_g) st[j] = ln_piece<C4>(st[j], *reinterpret_cast<const floatx4*>(ln_g + 4 * c4), eps);
                if constexpr (PAIR) {
                    const f16x4 hi = __builtin_convertvector(st[j], f16x4);
                    const f16x4 lo = __builtin_convertvector(st[j] - __builtin_convertvector(hi, floatx4), f16x4);
                    char* dst = reinterpret_cast<char*>(qo_smem) + row * RBX + 8 * c4;
                    *reinterpret_cast<f16x4*>(dst) = hi;
                    *reinterpret_cast<f16x4*>(dst + TP * RBX) = lo;
                } else if constexpr (TRI) {   // three bf16 planes (the arithmetic of split_triples_kernel)
                    const bf16x4 p0 = __builtin_convertvector(st[j], bf16x4);
                    const floatx4 r1 = st[j] - __builtin_convertvector(p0, floatx4);
                    const bf16x4 p1 = __builtin_convertvector(r1, bf16x4);
                    const bf16x4 p2 = __builtin_convertvector(r1 - __builtin_convertvector(p1, floatx4), bf16x4);
                    char* dst = reinterpret_cast<char*>(qo_smem) + row * RBX + 8 * c4;
                    *reinterpret_cast<bf16x4*>(dst) = p0;
                    *reinterpret_cast<bf16x4*>(dst + TP * RBX) = p1;
                    *reinterpret_cast<bf16x4*>(dst + 2 * TP * RBX) = p2;
                } else if constexpr (P16) {   // one plane, RNE
                    *reinterpret_cast<typename M16::x4*>(reinterpret_cast<char*>(qo_smem) + row * RBX + 8 * c4) = __builtin_convertvector(st[j], typename M16::x4);
                } else {
                    *reinterpret_cast<floatx4*>(Xs + row * LDA + 4 * c4) = st[j];
                }
            }
        }
    };
    auto stage_tile_bf = [&](auto full_tag) {
        constexpr bool FULL = decltype(full_tag)::value;
        const char* xb = reinterpret_cast<const char*>(xn);
        const char* slab_in = xb + (img + t0 + wave * 32) * C * 2;
        constexpr int NB = NQ8 < 8 ? NQ8 : 8;
#pragma unroll
        for (int j0 = 0; j0 < NQ8; j0 += NB) {
            bf16x8 st[NB];
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const int i = lane + 64 * (j0 + j), row = wave * 32 + lane / C8 + (64 / C8) * (j0 + j), c8 = lane % C8;   // (C8 divides 64)
                if constexpr (FULL) st[j] = *reinterpret_cast<const bf16x8*>(slab_in + 16 * (size_t)i);
                else st[j] = *reinterpret_cast<const bf16x8*>(xb + ((img + min(t0 + row, N - 1)) * C + 8 * c8) * 2);
                if constexpr (FULL && KEEP8) xkeep8[j0 + j] = st[j];
            }
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const int row = wave * 32 + lane / C8 + (64 / C8) * (j0 + j), c8 = lane % C8;
                if (ln_g) st[j] = __builtin_convertvector(ln_piece8<C8>(__builtin_convertvector(st[j], floatx8), ln_g + 8 * c8, eps), bf16x8);
                *reinterpret_cast<bf16x8*>(reinterpret_cast<char*>(qo_smem) + row * RBX + 16 * c8) = st[j];
            }
        }
    };
    // TRI: a K step of phase B is 12 MFMAs of 32 cycles — less than one L2 round trip — so the Wq fragments (three planes) run DB K steps ahead in a ring of
    // DB + 1 slots, and the ring's opening loads go out in front of the staging, which hides them (they do not depend on the tile)
    constexpr int NKB = C / 16, DB = TRI ? (NKB - 1 < 3 ? NKB - 1 : 3) : 0;
    [[maybe_unused]] bf16x8 wq3[DB + 1][3];
    [[maybe_unused]] const char* wq3row = TRI ? reinterpret_cast<const char*>(wq_pair) + ((size_t)wave * (C / 16) * 64 + 32 * h + l31) * 16 : nullptr;   // wq_pair: three planes of [128][C] in fragment order (attn_frag3_index), row tile = head
    constexpr size_t WQPL = (size_t)kHid * C * 2;   // bytes between two planes of Wq
    if constexpr (TRI) {
#pragma unroll
        for (int pf = 0; pf < DB; ++pf)
#pragma unroll
            for (int p = 0; p < 3; ++p) wq3[pf][p] = *reinterpret_cast<const bf16x8*>(wq3row + p * WQPL + 1024 * pf);
        __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (ABF) {
        if (full_tile) stage_tile_bf(std::true_type{}); else stage_tile_bf(std::false_type{});
    } else {
        if (full_tile) stage_tile(std::true_type{}); else stage_tile(std::false_type{});
    }
    // context operand of phase D: ctx[d = (s&3) + 8(s>>2) + 4h][e = l31] of head = wave
    float cb[16];
    {
        const float* cp = ctx + ((size_t)(b * kHeads + wave)) * 1024 + l31;
#pragma unroll
        for (int s2 = 0; s2 < 16; ++s2) cb[s2] = cp[((s2 & 3) + 8 * (s2 >> 2) + 4 * h) * 32];
    }
    // fp16 operands (MODE 3): the context carries v / N (module_util.py:168) — O(1e-6) on a 256 x 256 map, in fp16's subnormal range — so it and with it the
    // attention output go through the 16-bit MFMAs scaled by ctx_up = 2^ceil(log2 N) (exact), undone on the to_out accumulators in front of the bias.
    // fp16 pairs (MODE 1) the same: unscaled, the lo piece of an attention output of O(1 / N) falls into fp16's subnormal range (absolute spacing 2^-24) and the
    // pair loses its 22 bits — a relative error of the block that grows with N (2e-4 of the branch at 520 pixels; tests/test_gpu_linear_attn.py found it)
    float ctx_up = 1.f;
    if constexpr (MODE == AttnMode::Fp16 || PAIR) {
        ctx_up = exp2f(ceilf(log2f((float)N)));
#pragma unroll
        for (int s2 = 0; s2 < 16; ++s2) cb[s2] *= ctx_up;
    }
    __syncthreads();

    // ---- B: Q^T of head = wave
    floatx16 q[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) q[ct][r] = 0.f;
    if constexpr (PAIR) {
        const char* wrow = reinterpret_cast<const char*>(wq_pair) + ((size_t)(wave * kDh + l31) * C + 8 * h) * 2;
        constexpr size_t WPL = (size_t)kHid * C * 2;   // bytes between the hi and the lo plane of Wq
        const char* brow = reinterpret_cast<const char*>(qo_smem) + l31 * RBX + 16 * h;
        constexpr int NK16 = C / 16;
        f16x8 wa2[2][2];
        wa2[0][0] = *reinterpret_cast<const f16x8*>(wrow);
        wa2[0][1] = *reinterpret_cast<const f16x8*>(wrow + WPL);
#pragma unroll
        for (int ks = 0; ks < NK16; ++ks) {
            const int cur = ks & 1, nxt = cur ^ 1;
            const int kp = (ks + 1 < NK16 ? ks + 1 : ks) * 32;
            wa2[nxt][0] = *reinterpret_cast<const f16x8*>(wrow + kp);
            wa2[nxt][1] = *reinterpret_cast<const f16x8*>(wrow + WPL + kp);
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const f16x8 bh = *reinterpret_cast<const f16x8*>(brow + ct * 32 * RBX + 32 * ks);
                const f16x8 bl = *reinterpret_cast<const f16x8*>(brow + TP * RBX + ct * 32 * RBX + 32 * ks);
                q[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wa2[cur][0], bl, q[ct], 0, 0, 0);
                q[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wa2[cur][1], bh, q[ct], 0, 0, 0);
                q[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wa2[cur][0], bh, q[ct], 0, 0, 0);
            }
        }
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) q[ct][r] *= wq_inv;
    } else if constexpr (TRI) {
        // three pieces, six products (x0 w2, x1 w1, x2 w0, x0 w1, x1 w0, x0 w0: smallest first)
        const char* brow = reinterpret_cast<const char*>(qo_smem) + l31 * RBX + 16 * h;
#pragma unroll
        for (int ks = 0; ks < NKB; ++ks) {
            if (ks + DB < NKB) {
#pragma unroll
                for (int p = 0; p < 3; ++p) wq3[(ks + DB) % (DB + 1)][p] = *reinterpret_cast<const bf16x8*>(wq3row + p * WQPL + 1024 * (ks + DB));
            }
            __builtin_amdgcn_sched_barrier(0);  // keep the prefetch in front of this step's MFMAs
            const bf16x8* wa3c = wq3[ks % (DB + 1)];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(brow + ct * 32 * RBX + 32 * ks);
                const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(brow + TP * RBX + ct * 32 * RBX + 32 * ks);
                const bf16x8 b2 = *reinterpret_cast<const bf16x8*>(brow + 2 * TP * RBX + ct * 32 * RBX + 32 * ks);
                q[ct] = M16::mfma(wa3c[2], b0, q[ct]);
                q[ct] = M16::mfma(wa3c[1], b1, q[ct]);
                q[ct] = M16::mfma(wa3c[0], b2, q[ct]);
                q[ct] = M16::mfma(wa3c[1], b0, q[ct]);
                q[ct] = M16::mfma(wa3c[0], b1, q[ct]);
                q[ct] = M16::mfma(wa3c[0], b0, q[ct]);
            }
        }
    } else if constexpr (P16) {
        using x8 = typename M16::x8;
        const char* wrow = reinterpret_cast<const char*>(wq_pair) + ((size_t)(wave * kDh + l31) * C + 8 * h) * 2;
        const char* brow = reinterpret_cast<const char*>(qo_smem) + l31 * RBX + 16 * h;
        constexpr int NK16 = C / 16;
        x8 wa1[2];
        wa1[0] = *reinterpret_cast<const x8*>(wrow);
#pragma unroll
        for (int ks = 0; ks < NK16; ++ks) {
            const int cur = ks & 1, nxt = cur ^ 1;
            wa1[nxt] = *reinterpret_cast<const x8*>(wrow + (ks + 1 < NK16 ? ks + 1 : ks) * 32);
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)
                q[ct] = M16::mfma(wa1[cur], *reinterpret_cast<const x8*>(brow + ct * 32 * RBX + 32 * ks), q[ct]);
        }
    } else
    {
        const float* wrow = wq + (size_t)(wave * kDh + l31) * C + 4 * h;
        const float* brow = Xs + l31 * LDA + 4 * h;
        // weight fragments two K steps (32 MFMAs) ahead of their use: they come from L2
        constexpr int NK = C / 8;
        floatx4 wa[3];
        wa[0] = *reinterpret_cast<const floatx4*>(wrow);
        wa[1] = *reinterpret_cast<const floatx4*>(wrow + 8);
#pragma unroll
        for (int ks = 0; ks < NK; ++ks) {
            if (ks + 2 < NK) wa[(ks + 2) % 3] = *reinterpret_cast<const floatx4*>(wrow + 8 * (ks + 2));
            __builtin_amdgcn_sched_barrier(0);  // keep the prefetch in front of this step's MFMAs (the scheduler sinks it to its use)
            const floatx4 a = wa[ks % 3];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const floatx4 bb = *reinterpret_cast<const floatx4*>(brow + ct * 32 * LDA + 8 * ks);
                q[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bb.x, q[ct], 0, 0, 0);
                q[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bb.y, q[ct], 0, 0, 0);
                q[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bb.z, q[ct], 0, 0, 0);
                q[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bb.w, q[ct], 0, 0, 0);
            }
        }
    }
    // TRI: the to_out fragments of phase F (a K step there is 6 RTW MFMAs) run DF K steps ahead — the whole K range at C = 64; the ring's opening loads go out
    // here, in front of phases C - E, which hide them
    constexpr int RTW = TRI ? RT / 2 : RT;
    constexpr int NKF = kHid / 16, DF = !TRI ? 0 : RTW == 1 ? NKF - 1 : RTW == 2 ? 3 : 1;
    const int rt0 = TRI ? (wave >> 1) * RTW : 0;          // first 32-channel row tile of this wave (phases F, G)
    const int prow = TRI ? (wave & 1) * 32 : wave * 32;   // first pixel row (of the tile) of this wave (phases F, G)
    [[maybe_unused]] bf16x8 wo3[DF + 1][3][TRI ? RTW : 1];
    [[maybe_unused]] const char* wo3row = TRI ? reinterpret_cast<const char*>(wout_pair) + ((size_t)rt0 * (kHid / 16) * 64 + 32 * h + l31) * 16 : nullptr;   // wout_pair: three planes of [C][128] in fragment order
    constexpr size_t WOPL = (size_t)C * kHid * 2;   // bytes between two planes of Wout
    if constexpr (TRI) {
#pragma unroll
        for (int pf = 0; pf < DF; ++pf)
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
                for (int rt = 0; rt < RTW; ++rt) wo3[pf][p][rt] = *reinterpret_cast<const bf16x8*>(wo3row + p * WOPL + (size_t)rt * 32 * kHid * 2 + 1024 * pf);
        __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();  // every wave is done reading Xs: the region becomes Os
    // ---- C + D + E per pixel tile: q[ct][r] = Q[d = (r&3) + 8(r>>2) + 4h][pixel 32 ct + l31]
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        float m = q[ct][0];
#pragma unroll
        for (int r = 1; r < 16; ++r) m = fmaxf(m, q[ct][r]);
        m = half_max(m);
        float z = 0.f;
        const float ml = m * 1.44269504088896341f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            q[ct][r] = __builtin_amdgcn_exp2f(__builtin_fmaf(q[ct][r], 1.44269504088896341f, -ml));  // (the factor of m's rounding cancels in / z)
            z += q[ct][r];
        }
        z = half_sum(z);
        const float iz = __builtin_amdgcn_rcpf(z);   // v_rcp_f32 (1 ulp): softmax normalisation
        floatx16 o;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] = 0.f;
        if constexpr (MODE == AttnMode::Bf16 || MODE == AttnMode::Fp16) {
            // 16-bit operand modes: the context operand (rounded once per block) and the softmax probabilities (in [0, 1]) on the 16-bit MFMA, fp32
            // accumulation.  K step sh = the d values of the lane's registers 8 sh .. 8 sh + 7, the same order in cb[] and q[]: 2 MFMAs instead of 16.
            using x8 = typename M16::x8;
#pragma unroll
            for (int sh = 0; sh < 2; ++sh) {
                // (MODE 3: cb carries the power of two `ctx_up`, see above)
                const floatx8 ca = {cb[8 * sh], cb[8 * sh + 1], cb[8 * sh + 2], cb[8 * sh + 3], cb[8 * sh + 4], cb[8 * sh + 5], cb[8 * sh + 6], cb[8 * sh + 7]};
                const floatx8 qa = {q[ct][8 * sh], q[ct][8 * sh + 1], q[ct][8 * sh + 2], q[ct][8 * sh + 3],
                                    q[ct][8 * sh + 4], q[ct][8 * sh + 5], q[ct][8 * sh + 6], q[ct][8 * sh + 7]};
                o = M16::mfma(__builtin_convertvector(ca, x8), __builtin_convertvector(qa * iz, x8), o);
            }
        } else {
#pragma unroll
            for (int s2 = 0; s2 < 16; ++s2) o = __builtin_amdgcn_mfma_f32_32x32x2f32(cb[s2], q[ct][s2] * iz, o, 0, 0, 0);
        }
        // o[r] = out[pixel 32 ct + l31][e = (r&3) + 8(r>>2) + 4h]: four 16-byte groups per lane
        if constexpr (PAIR) {
            char* orow = reinterpret_cast<char*>(qo_smem) + (ct * 32 + l31) * RBO + (wave * kDh + 4 * h) * 2;
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const floatx4 v = floatx4{o[4 * gq], o[4 * gq + 1], o[4 * gq + 2], o[4 * gq + 3]};
                const f16x4 hi = __builtin_convertvector(v, f16x4);
                const f16x4 lo = __builtin_convertvector(v - __builtin_convertvector(hi, floatx4), f16x4);
                *reinterpret_cast<f16x4*>(orow + 16 * gq) = hi;
                *reinterpret_cast<f16x4*>(orow + TP * RBO + 16 * gq) = lo;
            }
        } else if constexpr (TRI) {
            char* orow = reinterpret_cast<char*>(qo_smem) + (ct * 32 + l31) * RBO + (wave * kDh + 4 * h) * 2;
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const floatx4 v = floatx4{o[4 * gq], o[4 * gq + 1], o[4 * gq + 2], o[4 * gq + 3]};
                const bf16x4 p0 = __builtin_convertvector(v, bf16x4);
                const floatx4 r1 = v - __builtin_convertvector(p0, floatx4);
                const bf16x4 p1 = __builtin_convertvector(r1, bf16x4);
                const bf16x4 p2 = __builtin_convertvector(r1 - __builtin_convertvector(p1, floatx4), bf16x4);
                *reinterpret_cast<bf16x4*>(orow + 16 * gq) = p0;
                *reinterpret_cast<bf16x4*>(orow + TP * RBO + 16 * gq) = p1;
                *reinterpret_cast<bf16x4*>(orow + 2 * TP * RBO + 16 * gq) = p2;
            }
        } else if constexpr (P16) {
            char* orow = reinterpret_cast<char*>(qo_smem) + (ct * 32 + l31) * RBO + (wave * kDh + 4 * h) * 2;
#pragma unroll
            for (int gq = 0; gq < 4; ++gq)
                *reinterpret_cast<typename M16::x4*>(orow + 16 * gq) =
                    __builtin_convertvector(floatx4{o[4 * gq], o[4 * gq + 1], o[4 * gq + 2], o[4 * gq + 3]}, typename M16::x4);
        } else {
            float* orow = Os + (ct * 32 + l31) * LDO + wave * kDh + 4 * h;
#pragma unroll
            for (int gq = 0; gq < 4; ++gq)
                *reinterpret_cast<floatx4*>(orow + 8 * gq) = floatx4{o[4 * gq], o[4 * gq + 1], o[4 * gq + 2], o[4 * gq + 3]};
        }
    }
    __syncthreads();  // Os complete

    // ---- F: y^T[c][px] of the 32-pixel tile = wave
    // TRI (64-pixel tile = two 32-pixel tiles): wave = (pixel tile wave & 1) x (half of the output channels wave >> 1) — RTW = RT / 2 row tiles of 32 channels per wave;
    // the LayerNorm sums of phase G then span two waves and are exchanged through LDS
    floatx16 yv[RTW];
#pragma unroll
    for (int rt = 0; rt < RTW; ++rt)
#pragma unroll
        for (int r = 0; r < 16; ++r) yv[rt][r] = 0.f;
    if constexpr (TRI) {
        // six products per K step of 16 (o0 w2, o1 w1, o2 w0, o0 w1, o1 w0, o0 w0: smallest first)
        const char* brow = reinterpret_cast<const char*>(qo_smem) + (prow + l31) * RBO + 16 * h;
#pragma unroll
        for (int ks = 0; ks < NKF; ++ks) {
            if (ks + DF < NKF) {
#pragma unroll
                for (int p = 0; p < 3; ++p)
#pragma unroll
                    for (int rt = 0; rt < RTW; ++rt)
                        wo3[(ks + DF) % (DF + 1)][p][rt] = *reinterpret_cast<const bf16x8*>(wo3row + p * WOPL + (size_t)rt * 32 * kHid * 2 + 1024 * (ks + DF));
            }
            __builtin_amdgcn_sched_barrier(0);
            const auto& wa3c = wo3[ks % (DF + 1)];
            const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(brow + 32 * ks);
            const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(brow + TP * RBO + 32 * ks);
            const bf16x8 b2 = *reinterpret_cast<const bf16x8*>(brow + 2 * TP * RBO + 32 * ks);
#pragma unroll
            for (int rt = 0; rt < RTW; ++rt) yv[rt] = M16::mfma(wa3c[2][rt], b0, yv[rt]);
#pragma unroll
            for (int rt = 0; rt < RTW; ++rt) yv[rt] = M16::mfma(wa3c[1][rt], b1, yv[rt]);
#pragma unroll
            for (int rt = 0; rt < RTW; ++rt) yv[rt] = M16::mfma(wa3c[0][rt], b2, yv[rt]);
#pragma unroll
            for (int rt = 0; rt < RTW; ++rt) yv[rt] = M16::mfma(wa3c[1][rt], b0, yv[rt]);
#pragma unroll
            for (int rt = 0; rt < RTW; ++rt) yv[rt] = M16::mfma(wa3c[0][rt], b1, yv[rt]);
#pragma unroll
            for (int rt = 0; rt < RTW; ++rt) yv[rt] = M16::mfma(wa3c[0][rt], b0, yv[rt]);
        }
    } else if constexpr (PAIR) {
        const char* wrow = reinterpret_cast<const char*>(wout_pair) + ((size_t)l31 * kHid + 8 * h) * 2;
        constexpr size_t WPL = (size_t)C * kHid * 2;   // bytes between the hi and the lo plane of Wout
        const char* brow = reinterpret_cast<const char*>(qo_smem) + (wave * 32 + l31) * RBO + 16 * h;
        constexpr int NK16 = kHid / 16;
        // r06: C = 256 (RT = 8 row tiles) walks its row tiles in two halves: 128 accumulators + a double-buffered fragment pair per row tile of ALL eight
        // was 256 + registers (177 spilled to scratch); per accumulator the products arrive in the same order (bit-identical)
        constexpr int RH = RT > 4 ? RT / 4 : RT;
#pragma unroll
        for (int r0 = 0; r0 < RT; r0 += RH) {
            f16x8 wa2[2][2][RH];
#pragma unroll
            for (int rt = 0; rt < RH; ++rt) {
                wa2[0][0][rt] = *reinterpret_cast<const f16x8*>(wrow + (size_t)(r0 + rt) * 32 * kHid * 2);
                wa2[0][1][rt] = *reinterpret_cast<const f16x8*>(wrow + WPL + (size_t)(r0 + rt) * 32 * kHid * 2);
            }
#pragma unroll
            for (int ks = 0; ks < NK16; ++ks) {
                const int cur = ks & 1, nxt = cur ^ 1;
                const int kp = (ks + 1 < NK16 ? ks + 1 : ks) * 32;
#pragma unroll
                for (int rt = 0; rt < RH; ++rt) {
                    wa2[nxt][0][rt] = *reinterpret_cast<const f16x8*>(wrow + (size_t)(r0 + rt) * 32 * kHid * 2 + kp);
                    wa2[nxt][1][rt] = *reinterpret_cast<const f16x8*>(wrow + WPL + (size_t)(r0 + rt) * 32 * kHid * 2 + kp);
                }
                const f16x8 bh = *reinterpret_cast<const f16x8*>(brow + 32 * ks);
                const f16x8 bl = *reinterpret_cast<const f16x8*>(brow + TP * RBO + 32 * ks);
#pragma unroll
                for (int rt = 0; rt < RH; ++rt) yv[r0 + rt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wa2[cur][0][rt], bl, yv[r0 + rt], 0, 0, 0);
#pragma unroll
                for (int rt = 0; rt < RH; ++rt) yv[r0 + rt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wa2[cur][1][rt], bh, yv[r0 + rt], 0, 0, 0);
#pragma unroll
                for (int rt = 0; rt < RH; ++rt) yv[r0 + rt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wa2[cur][0][rt], bh, yv[r0 + rt], 0, 0, 0);
            }
        }
        const float dn = wout_inv * (1.0f / ctx_up);   // two powers of two: the weights' scale and the context's
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r) yv[rt][r] *= dn;
    } else if constexpr (P16) {
        using x8 = typename M16::x8;
        const char* wrow = reinterpret_cast<const char*>(wout_pair) + ((size_t)l31 * kHid + 8 * h) * 2;
        const char* brow = reinterpret_cast<const char*>(qo_smem) + (wave * 32 + l31) * RBO + 16 * h;
        constexpr int NK16 = kHid / 16;
        x8 wa1[2][RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) wa1[0][rt] = *reinterpret_cast<const x8*>(wrow + (size_t)rt * 32 * kHid * 2);
#pragma unroll
        for (int ks = 0; ks < NK16; ++ks) {
            const int cur = ks & 1, nxt = cur ^ 1;
            const int kp = (ks + 1 < NK16 ? ks + 1 : ks) * 32;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) wa1[nxt][rt] = *reinterpret_cast<const x8*>(wrow + (size_t)rt * 32 * kHid * 2 + kp);
            const x8 bb = *reinterpret_cast<const x8*>(brow + 32 * ks);
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) yv[rt] = M16::mfma(wa1[cur][rt], bb, yv[rt]);
        }
        if constexpr (MODE == AttnMode::Fp16) {
            const float dn = 1.0f / ctx_up;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int r = 0; r < 16; ++r) yv[rt][r] *= dn;
        }
    } else
    {
        const float* wrow = wout + (size_t)l31 * kHid + 4 * h;
        const float* brow = Os + (wave * 32 + l31) * LDO + 4 * h;
        // to_out weight fragments (RT per K step, from L2) PF K steps ahead of their use (C = 256: one step = 32 MFMAs already,
        // and eight fragments per step leave no registers for a deeper ring)
        constexpr int NK = kHid / 8;
        constexpr int PF = RT > 4 ? 1 : 2, RING = PF + 1;
        floatx4 wa[RING][RT];
#pragma unroll
        for (int pf = 0; pf < PF; ++pf)
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) wa[pf][rt] = *reinterpret_cast<const floatx4*>(wrow + (size_t)rt * 32 * kHid + 8 * pf);
#pragma unroll
        for (int ks = 0; ks < NK; ++ks) {
            if (ks + PF < NK) {
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
                    wa[(ks + PF) % RING][rt] = *reinterpret_cast<const floatx4*>(wrow + (size_t)rt * 32 * kHid + 8 * (ks + PF));
            }
            __builtin_amdgcn_sched_barrier(0);
            const floatx4 bb = *reinterpret_cast<const floatx4*>(brow + 8 * ks);
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const floatx4 a = wa[ks % RING][rt];
                yv[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bb.x, yv[rt], 0, 0, 0);
                yv[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bb.y, yv[rt], 0, 0, 0);
                yv[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bb.z, yv[rt], 0, 0, 0);
                yv[rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bb.w, yv[rt], 0, 0, 0);
            }
        }
    }
    // ---- G: bias, LayerNorm over the C channels of pixel 32 wave + l31 (this lane holds c = 32 rt + (r&3) + 8(r>>2) + 4h)
    float sum = 0.f;
#pragma unroll
    for (int rt = 0; rt < RTW; ++rt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            yv[rt][r] += bias[32 * (rt0 + rt) + (r & 3) + 8 * (r >> 2) + 4 * h];
            sum += yv[rt][r];
        }
    sum = half_sum(sum);
    // TRI: the other half of the pixel's channels sits in wave ^ 2 — partial sums through LDS (behind the planes; added in a fixed order: deterministic)
    [[maybe_unused]] float* red = reinterpret_cast<float*>(reinterpret_cast<char*>(qo_smem) + qo_tri_main_bytes(C));   // [sum | sq][channel half][64 pixels]
    if constexpr (TRI) {
        if (h == 0) red[(wave >> 1) * TP + prow + l31] = sum;
        __syncthreads();   // (every wave has left phase F: the region is free for the normalised rows below)
        sum = red[prow + l31] + red[TP + prow + l31];
    }
    const float mean = sum * (1.0f / (float)C);
    float sq = 0.f;
#pragma unroll
    for (int rt = 0; rt < RTW; ++rt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            yv[rt][r] -= mean;
            sq += yv[rt][r] * yv[rt][r];
        }
    sq = half_sum(sq);
    if constexpr (TRI) {
        if (h == 0) red[2 * TP + (wave >> 1) * TP + prow + l31] = sq;
        __syncthreads();
        sq = red[2 * TP + prow + l31] + red[3 * TP + prow + l31];
    }
    const float rstd = __builtin_amdgcn_rsqf(sq * (1.0f / (float)C) + eps);
    // Ys = this wave's own 32 rows of the region.  C <= 128: row stride LDO, exactly the Os rows only this wave read in phase F.
    // C = 256: the rows are wider than an Os row, so they overlap other waves' Os rows -> wait until every wave has left phase F.
    // PAIR: the fp16 planes put other waves' Os rows inside this wave's Ys rows for every C -> always wait.
    if constexpr (!TRI && (C > kHid || P16)) __syncthreads();
    float* yrow = Os + (prow + l31) * LDY + 32 * rt0 + 4 * h;
#pragma unroll
    for (int rt = 0; rt < RTW; ++rt)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const floatx4 g4 = *reinterpret_cast<const floatx4*>(g2 + 32 * (rt0 + rt) + 8 * gq + 4 * h);
            *reinterpret_cast<floatx4*>(yrow + 32 * rt + 8 * gq) =
                floatx4{yv[rt][4 * gq] * rstd * g4.x, yv[rt][4 * gq + 1] * rstd * g4.y, yv[rt][4 * gq + 2] * rstd * g4.z,
                        yv[rt][4 * gq + 3] * rstd * g4.w};
        }
    // the wave re-reads only its own rows: LDS operations of one wave complete in order, no block barrier needed
    // (TRI: a wave stores the 16-row slab it staged, which four waves normalised -> block barrier)
    if constexpr (TRI) __syncthreads();
    else __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
    auto residual_store = [&](auto full_tag) {
        constexpr bool FULL = decltype(full_tag)::value;
        const size_t slab = (img + t0 + wave * SL) * C;   // the wave's 32 rows are contiguous: element 4 i of the slab is piece i
        floatx4 xr[NQ];
        if (FULL && KEEP && keep_res) {
#pragma unroll
            for (int j = 0; j < NQ; ++j) xr[j] = xkeep[KEEP ? j : 0];   // the pieces staged in phase A
        } else {
#pragma unroll
            for (int j = 0; j < NQ; ++j) {  // residual loads first, all in flight
                const int i = lane + 64 * j, row = lane / C4 + (64 / C4) * j, c4 = lane % C4;   // (C4 divides 64)
                if constexpr (FULL) xr[j] = *reinterpret_cast<const floatx4*>(xres + slab + 4 * i);
                else xr[j] = *reinterpret_cast<const floatx4*>(xres + (img + min(t0 + wave * SL + row, N - 1)) * C + 4 * c4);
            }
        }
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const int i = lane + 64 * j, row = lane / C4 + (64 / C4) * j, c4 = lane % C4;   // (C4 divides 64)
            const int n = t0 + wave * SL + row;
            const floatx4 v = *reinterpret_cast<const floatx4*>(Os + (wave * SL + row) * LDY + 4 * c4);
            if constexpr (FULL) *reinterpret_cast<floatx4*>(y + slab + 4 * i) = v + xr[j];
            else if (n < N) *reinterpret_cast<floatx4*>(y + (img + n) * C + 4 * c4) = v + xr[j];
        }
    };
    // ABF: residual and output are bf16 rows; the sum is formed in fp32 and rounded once (RNE)
    auto residual_store_bf = [&](auto full_tag) {
        constexpr bool FULL = decltype(full_tag)::value;
        const char* rb = reinterpret_cast<const char*>(xres);
        char* yb = reinterpret_cast<char*>(y);
        const size_t slab = (img + t0 + wave * 32) * C * 2;   // byte offset of the wave's 32 contiguous rows
        bf16x8 xr[NQ8];
        if (FULL && KEEP8 && keep_res) {
#pragma unroll
            for (int j = 0; j < NQ8; ++j) xr[j] = xkeep8[KEEP8 ? j : 0];
        } else {
#pragma unroll
            for (int j = 0; j < NQ8; ++j) {
                const int i = lane + 64 * j, row = lane / C8 + (64 / C8) * j, c8 = lane % C8;
                if constexpr (FULL) xr[j] = *reinterpret_cast<const bf16x8*>(rb + slab + 16 * (size_t)i);
                else xr[j] = *reinterpret_cast<const bf16x8*>(rb + ((img + min(t0 + wave * 32 + row, N - 1)) * C + 8 * c8) * 2);
            }
        }
#pragma unroll
        for (int j = 0; j < NQ8; ++j) {
            const int i = lane + 64 * j, row = lane / C8 + (64 / C8) * j, c8 = lane % C8;
            const int n = t0 + wave * 32 + row;
            const float* yr = Os + (wave * 32 + row) * LDY + 8 * c8;
            const floatx4 va = *reinterpret_cast<const floatx4*>(yr), vb = *reinterpret_cast<const floatx4*>(yr + 4);
            const floatx8 v = floatx8{va.x, va.y, va.z, va.w, vb.x, vb.y, vb.z, vb.w} + __builtin_convertvector(xr[j], floatx8);
            const bf16x8 o = __builtin_convertvector(v, bf16x8);
            if constexpr (FULL) *reinterpret_cast<bf16x8*>(yb + slab + 16 * (size_t)i) = o;
            else if (n < N) *reinterpret_cast<bf16x8*>(yb + ((img + n) * C + 8 * c8) * 2) = o;
        }
    };
    if constexpr (ABF) {
        if (full_tile) residual_store_bf(std::true_type{}); else residual_store_bf(std::false_type{});
    } else {
        if (full_tile) residual_store(std::true_type{}); else residual_store(std::false_type{});
    }
}

}  // namespace

// pixels per context chunk: 32 chunks per image, more for small batches so that the chunk grid (chunks x B blocks) still fills
// the 256 CUs (r03: at B = 2 the 64-block k/v kernels ran 4-5x slower per image than at B = 16); never below one 128-pixel tile
int attn_chunk_len(int N, int B) {
    const int want = std::max(32, (512 + B - 1) / std::max(B, 1));
    int len = (N + want - 1) / want;
    if (len < 128) len = 128;
    return (len + 7) & ~7;
}
int attn_num_chunks(int N, int B) {
    const int len = attn_chunk_len(N, B);
    return (N + len - 1) / len;
}

// ---------------------------------------------------------------------------------------------
// The instances of the two fused kernels.  These two lists are the only place that names them: the dynamic-LDS attribute, the kernel and the LDS bytes of a
// launch and attn_fused_has_instance() (the plan builder's question) all read them, and a row that is not here is not compiled.
// ---------------------------------------------------------------------------------------------
namespace {

using M = AttnMode;
// Dynamic LDS of one block.  k / v context: the staged tile — f32 rows of C + 4 floats, or one / two / three 16-bit planes with rows of 2 C + 16 bytes.
constexpr size_t kv_lds_bytes(int C, AttnMode mode) {
    if (mode == M::F32) return (size_t)kKvTile * (C + 4) * sizeof(float);
    return (size_t)(mode == M::Bf16x3 ? 3 * kKvTileTri : mode == M::PairF16 ? 2 * kKvTile : kKvTile) * (2 * C + 16);
}
constexpr int qo_tile(AttnMode mode) { return mode == M::Bf16x3 ? kQoTileTri : 128; }   // pixels per block
// q + out: one region = max(xn planes, attention-output planes, f32 out tile); the three-piece mode adds its LayerNorm partial sums
constexpr size_t qo_lds_bytes(int C, AttnMode mode) {
    if (mode == M::Bf16x3) return qo_tri_main_bytes(C) + (size_t)4 * kQoTileTri * sizeof(float);
    const size_t ys = (size_t)128 * ((C > kHid ? C : kHid) + 4) * sizeof(float);
    if (mode == M::F32) return ys;
    const size_t planes = mode == M::PairF16 ? 2 : 1;
    return std::max(std::max(planes * 128 * (2 * C + 16), planes * 128 * (2 * kHid + 16)), ys);
}
constexpr size_t kAttnMaxLds = 160 * 1024;

template <typename K>
struct AttnInst { int C; AttnMode mode; bool act_bf16; size_t lds; K kernel; };
using KvInst = AttnInst<decltype(&attn_kv_ctx_kernel<64, M::F32, false>)>;
using QoInst = AttnInst<decltype(&attn_q_out_fused_kernel<64, M::F32, false>)>;
template <int C, AttnMode MODE, bool ABF = false>
constexpr KvInst kv() {
    static_assert(kv_lds_bytes(C, MODE) <= kAttnMaxLds, "the tile does not fit the 160 KB of LDS");
    return {C, MODE, ABF, kv_lds_bytes(C, MODE), &attn_kv_ctx_kernel<C, MODE, ABF>};
}
template <int C, AttnMode MODE, bool ABF = false>
constexpr QoInst qo() {
    static_assert(qo_lds_bytes(C, MODE) <= kAttnMaxLds, "the tile does not fit the 160 KB of LDS");
    return {C, MODE, ABF, qo_lds_bytes(C, MODE), &attn_q_out_fused_kernel<C, MODE, ABF>};
}
constexpr KvInst kKvInst[] = {
    kv<32, M::F32>(), kv<64, M::F32>(), kv<96, M::F32>(), kv<128, M::F32>(), kv<160, M::F32>(), kv<192, M::F32>(), kv<224, M::F32>(), kv<256, M::F32>(),
    kv<64, M::PairF16>(), kv<128, M::PairF16>(), kv<256, M::PairF16>(),
    kv<64, M::Bf16>(), kv<128, M::Bf16>(), kv<256, M::Bf16>(),
    kv<64, M::Bf16, true>(), kv<128, M::Bf16, true>(), kv<256, M::Bf16, true>(),
    kv<64, M::Fp16>(), kv<128, M::Fp16>(), kv<256, M::Fp16>(),
    kv<64, M::Bf16x3>(), kv<128, M::Bf16x3>(), kv<256, M::Bf16x3>(),
};
constexpr QoInst kQoInst[] = {
    qo<64, M::F32>(), qo<128, M::F32>(), qo<256, M::F32>(),
    qo<64, M::PairF16>(), qo<128, M::PairF16>(), qo<256, M::PairF16>(),
    qo<64, M::Bf16>(), qo<128, M::Bf16>(), qo<256, M::Bf16>(),
    qo<64, M::Bf16, true>(), qo<128, M::Bf16, true>(), qo<256, M::Bf16, true>(),
    qo<64, M::Fp16>(), qo<128, M::Fp16>(), qo<256, M::Fp16>(),
    qo<64, M::Bf16x3>(), qo<128, M::Bf16x3>(), qo<256, M::Bf16x3>(),
};

template <typename Inst, size_t NI>
const Inst* find_inst(const Inst (&rows)[NI], int C, AttnMode mode, bool act_bf16) {
    for (const Inst& r : rows)
        if (r.C == C && r.mode == mode && r.act_bf16 == act_bf16) return &r;
    return nullptr;
}
// the table row of a launch; throws for a projection without its planes and for a shape the mode has no kernel for
template <typename Inst, size_t NI>
const Inst& pick_inst(const std::string& who, const Inst (&rows)[NI], int C, const AttnProj& p, bool has_planes) {
    static const char* const name[] = {"f32", "fp16-pair", "bf16", "fp16", "three-piece bf16"};
    const std::string mode = name[(int)p.mode];
    if (p.mode != M::F32 && !has_planes) throw HipError(who + ": the " + mode + " projection needs its weight planes");
    if (p.act_bf16 && p.mode != M::Bf16) throw HipError(who + ": bf16 activation storage goes with bf16 operands");
    const Inst* r = find_inst(rows, C, p.mode, p.act_bf16);
    if (!r)
        throw HipError(who + ": no " + mode + " kernel for C = " + std::to_string(C) +
                       " (the f32 k / v context takes multiples of 32 up to 256, everything else C = 64, 128, 256)");
    return *r;
}

void launch_ctx_finalize(int B, int N, int nch, const AttnWorkspace& ws, hipStream_t s) {
    hipLaunchKernelGGL(attn_ctx_finalize_kernel, dim3(B * kHeads, 4), dim3(1024), 0, s, ws.pctx, ws.psum, ws.pmax, ws.ctx, nch,
                       1.0f / (float)N, 1.0f / sqrtf((float)kDh));
}

}  // namespace

bool attn_fused_has_instance(int C, AttnMode mode, bool act_bf16) {
    return find_inst(kKvInst, C, mode, act_bf16) && find_inst(kQoInst, C, mode, act_bf16);
}

// pick_inst's verdict on one launcher's table without a launch (the kernel-level hooks refuse with the launcher's own message)
void attn_require_instance(bool q_out, int C, AttnMode mode, bool act_bf16) {
    AttnProj p;
    p.mode = mode;
    p.act_bf16 = act_bf16;
    if (q_out) pick_inst("attention_q_out_fused", kQoInst, C, p, true);
    else pick_inst("attention_kv_context", kKvInst, C, p, true);
}

// what the two launchers read for one shape: table rows, LDS bytes, tiles and the chunk geometry (host only)
AttnChoice attn_choice(int C, AttnMode mode, bool act_bf16, int N, int B) {
    AttnChoice c;
    c.kv_rows = (int)(sizeof(kKvInst) / sizeof(kKvInst[0]));
    c.qo_rows = (int)(sizeof(kQoInst) / sizeof(kQoInst[0]));
    if (const KvInst* r = find_inst(kKvInst, C, mode, act_bf16)) { c.kv_row = (int)(r - kKvInst); c.kv_lds = r->lds; }
    if (const QoInst* r = find_inst(kQoInst, C, mode, act_bf16)) { c.qo_row = (int)(r - kQoInst); c.qo_lds = r->lds; }
    c.kv_tile = mode == M::Bf16x3 ? kKvTileTri : kKvTile;
    c.qo_tile = qo_tile(mode);
    c.chunk_len = attn_chunk_len(N, B);
    c.nch = attn_num_chunks(N, B);
    return c;
}

// > 64 KB of dynamic LDS needs the attribute on the CURRENT device: called from conv_global_init() (engine finalize, per
// engine and so per device, outside any stream capture) like every other kernel of the library
void attention_global_init() {
    for (const KvInst& r : kKvInst)
        IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(r.kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAttnMaxLds));
    for (const QoInst& r : kQoInst)
        IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(r.kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAttnMaxLds));
}

template <typename T>
static void linear_attention_t(const T* qkv, T* out, int B, int N, const AttnWorkspace& ws, hipStream_t s) {
    const int len = attn_chunk_len(N, B);
    const int nch = attn_num_chunks(N, B);
    if (nch != ws.nch) throw HipError("attention workspace chunk mismatch");
    hipLaunchKernelGGL(attn_ctx_partial_kernel<T>, dim3(nch, B * kHeads), dim3(256), 0, s, qkv, ws.pmax, ws.pctx, ws.psum,
                       N, len, nch);
    launch_ctx_finalize(B, N, nch, ws, s);
    const int tiles = (N + 31) / 32;
    hipLaunchKernelGGL(attn_out_kernel<T>, dim3((tiles + kOutTilesPerBlock - 1) / kOutTilesPerBlock, B), dim3(256), 0, s,
                       qkv, ws.ctx, out, N, kQkv);
    IRSDE_HIP_CHECK(hipGetLastError());
}
void launch_linear_attention(const float* qkv, float* out, int B, int N, const AttnWorkspace& ws, hipStream_t s, bool bf16) {
    if (bf16)
        linear_attention_t(reinterpret_cast<const bf16_t*>(qkv), reinterpret_cast<bf16_t*>(out), B, N, ws, s);
    else
        linear_attention_t(qkv, out, B, N, ws, s);
}

// context from xn and the k / v weight rows (attn_kv_ctx_kernel) + the merge of the chunks
void launch_attention_kv_context(const float* xn, const float* wkv, int B, int N, int C, const AttnWorkspace& ws, hipStream_t s,
                                 const float* ln_g, float ln_eps, const AttnProj& p) {
    if (ln_g && (C & (C - 1))) throw HipError("attention_kv_context: the fused LayerNorm needs a power-of-two channel count");
    const KvInst& r = pick_inst("attention_kv_context", kKvInst, C, p, p.kv != nullptr);
    const int len = attn_chunk_len(N, B);
    const int nch = attn_num_chunks(N, B);
    if (nch != ws.nch) throw HipError("attention workspace chunk mismatch");
    hipLaunchKernelGGL(r.kernel, dim3(nch, B), dim3(256), r.lds, s, xn, wkv, ws.pmax, ws.pctx, ws.psum, N, len, nch, ln_g, ln_eps, p.kv, p.kv_inv);
    launch_ctx_finalize(B, N, nch, ws, s);
    IRSDE_HIP_CHECK(hipGetLastError());
}
void launch_attention_q_out(const float* q, float* out, int B, int N, const AttnWorkspace& ws, hipStream_t s) {
    const int tiles = (N + 31) / 32;
    hipLaunchKernelGGL(attn_out_kernel<float>, dim3((tiles + kOutTilesPerBlock - 1) / kOutTilesPerBlock, B), dim3(256), 0, s, q, ws.ctx,
                       out, N, kHid);
    IRSDE_HIP_CHECK(hipGetLastError());
}

// y = LayerNorm(to_out(softmax(q) . ctx)) * g + x with q = Wq . xn computed in the kernel (C = 64, 128 or 256)
void launch_attention_q_out_fused(const float* xn, const float* x, const float* wq, const float* wout, const float* bias,
                                  const float* g2, float* y, int B, int N, int C, float eps, const AttnWorkspace& ws, hipStream_t s,
                                  const float* ln_g, const AttnProj& p) {
    const QoInst& r = pick_inst("attention_q_out_fused", kQoInst, C, p, p.q && p.out);
    const int tile = qo_tile(p.mode);
    hipLaunchKernelGGL(r.kernel, dim3((N + tile - 1) / tile, B), dim3(256), r.lds, s, xn, x, wq, ws.ctx, wout, bias, g2, y, N, eps, ln_g,
                       p.q, p.out, p.q_inv, p.out_inv);
    IRSDE_HIP_CHECK(hipGetLastError());
}

}  // namespace irsde
