// Stereo cross-attention module (SCAM) of the stereo-sr ConditionalNAFNet
// (codes/config/stereo-sr/models/modules/DenoisingNAFNet_arch.py:15-60) and the stereo input / output glue of that network.
//
// A SCAM on the block output x [2B][H][W][c] (NHWC, views stacked on the batch axis: [L_0..L_{B-1}, R_0..R_{B-1}]) runs as
//   1. scam_prologue_kernel   bicubic quarter-downsample + LayerNorm (norm_l / norm_r gain) -> xs2 [2B][H'][W'][LN(xs) | xs]
//   2. two 1x1 GEMMs           (the engine's implicit-GEMM kernel, one per view) against the block-diagonal [[proj1, 0], [0, proj2]]
//                              weight -> qv [2B][H'][W'][Q | V]
//   3. scam_core_kernel        per (pair, row, 16-row strip, direction): S strip on v_mfma_f32_16x16x4_f32 into LDS, exact softmax over
//                              the strip rows, P . V on the same MFMA -> F [2B][H'][W'][c]
//   4. scam_epilogue_kernel    out = x + scale[ch] * F[nearest(y), nearest(x)][ch]  (beta for the left view, gamma for the right)
// H' = floor(H / 4), W' = floor(W / 4).
//
// The core never holds the whole W' x W' score matrix: a work-group owns a 16 x W' strip (<= 33 KB of LDS at W' = 512).  Direction 0 takes
// strips of S = Q_l Q_r^T (rows i, softmax over j, times V_r: F_r2l); direction 1 takes strips of S^T = Q_r Q_l^T (rows j, softmax over i,
// times V_l: F_l2r).  Each strip sees its full rows, so both softmaxes are exact two-pass ones (max, then sum) with no running-max rescale;
// the price is that S is computed twice (once per direction), W'^2 c MACs on a 1/16-size map.  Every statistic and product is fp32.
//
// The stereo-sr ConditionalUNet (DenoisingUNet_arch.py:18-56) has a SCAM of its own behind every LinearAttention: the same two-way attention WITHOUT
// the quarter-downsample and the upsample, i.e. one W x W score matrix per image row at the level's full resolution (16 x the map of the NAFNet's).
// Its kernels are the *_full ones below: a LayerNorm-only prologue, scam_full_core_kernel and an in-place epilogue; the projections are the same
// block-diagonal GEMM.  The core keeps the 16 x W strip in LDS like scam_core_kernel, but walks k on the outside with one accumulator per column tile
// of the wave, so the strip's own Q rows are read once per wave instead of once per column tile; every row of the other view's Q / V is read by exactly
// one wave of the work-group.  Row width W <= kScamFullMaxW (1024: a 66 KB strip), c a multiple of 32 up to 2048.
#include "common.h"

namespace irsde {

namespace {

__device__ __forceinline__ float wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// PyTorch `F.interpolate(scale_factor=0.25, mode='bicubic', align_corners=False)`: output o samples at 4 o + 1.5, i.e. the cubic
// convolution (A = -0.75) at t = 0.5 over input rows / columns 4 o .. 4 o + 3: weights [-3, 19, 19, -3] / 32, no clamping needed.
__device__ __forceinline__ float bicubic_w(int k) { return (k == 0 || k == 3) ? -0.09375f : 0.59375f; }

// one wave per output pixel (n, h', w'); channel ch = lane + 64 q (c <= 1024: q < 16)
__global__ void __launch_bounds__(256) scam_prologue_kernel(const float* __restrict__ x, const float* __restrict__ g_l,
                                                            const float* __restrict__ g_r, float* __restrict__ xs2, int B, int H, int W,
                                                            int c, int Hs, int Ws) {
    const int lane = threadIdx.x & 63;
    const long long pix = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long npix = 2ll * B * Hs * Ws;
    if (pix >= npix) return;
    const int ws = (int)(pix % Ws);
    const int hs = (int)((pix / Ws) % Hs);
    const int n = (int)(pix / ((long long)Ws * Hs));
    const float* g = n < B ? g_l : g_r;
    const float* xb = x + (size_t)n * H * W * c;
    float v[16];
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int ch = lane + 64 * q;
        float acc = 0.f;
        if (ch < c) {
            for (int dy = 0; dy < 4; ++dy) {
                const float* row = xb + ((size_t)(4 * hs + dy) * W + 4 * ws) * c + ch;
                float r = 0.f;
                for (int dx = 0; dx < 4; ++dx) r += bicubic_w(dx) * row[(size_t)dx * c];
                acc += bicubic_w(dy) * r;
            }
        }
        v[q] = acc;
        sum += acc;
    }
    const float mean = wave_sum(sum) / (float)c;
    float sq = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int ch = lane + 64 * q;
        if (ch < c) {
            const float d = v[q] - mean;
            sq += d * d;
        }
    }
    const float rstd = rsqrtf(wave_sum(sq) / (float)c + 1e-5f);
    float* o = xs2 + (size_t)pix * 2 * c;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int ch = lane + 64 * q;
        if (ch < c) {
            o[ch] = (v[q] - mean) * rstd * g[ch];
            o[c + ch] = v[q];
        }
    }
}

using f32x4 = __attribute__((ext_vector_type(4))) float;

// grid (strips = ceil(W' / 16), B * H', 2 directions), 256 threads.  qv: [2B][H'][W'][Q (c) | V (c)], F: [2B][H'][W'][c].
// LDS: P[16][ld] (ld = Wt + 4, Wt = 16 ceil(W' / 16)) + inv[16].
__global__ void __launch_bounds__(256) scam_core_kernel(const float* __restrict__ qv, float* __restrict__ F, int B, int Hs, int Ws, int c,
                                                        float scale) {
    extern __shared__ float lds[];
    const int Wt = (Ws + 15) & ~15, ld = Wt + 4;
    float* P = lds;
    float* inv = lds + 16 * ld;
    const int strip = blockIdx.x, row = blockIdx.y, dir = blockIdx.z;
    const int b = row / Hs, h = row % Hs;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l16 = lane & 15, kk = lane >> 4;
    const size_t rowsz = (size_t)Ws * 2 * c;
    const int own_img = dir == 0 ? b : B + b, oth_img = dir == 0 ? B + b : b;
    const float* own = qv + ((size_t)own_img * Hs + h) * rowsz;   // strip rows: Q at [0, c)
    const float* oth = qv + ((size_t)oth_img * Hs + h) * rowsz;   // other view: Q at [0, c), V at [c, 2c)
    const int i0 = strip * 16;
    const int ntile = Wt / 16;

    // 1. S strip [16][Wt] = scale * Q_own[i0 .. i0 + 15] . Q_oth^T.  Lane (l16, kk) of k-block kb holds k = kb + 4 kk + s in MFMA step s for
    //    both operands, so every step multiplies matching k (any fixed k permutation shared by A and B leaves the sum over k unchanged).
    {
        const int ia = i0 + l16;
        const bool a_ok = ia < Ws;
        const float* arow = own + (size_t)(a_ok ? ia : 0) * 2 * c + 4 * kk;
        for (int t = wave; t < ntile; t += 4) {
            const int jb = t * 16 + l16;
            const bool b_ok = jb < Ws;
            const float* brow = oth + (size_t)(b_ok ? jb : 0) * 2 * c + 4 * kk;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            for (int k = 0; k < c; k += 32) {   // two k-blocks per trip (c is a multiple of 32): both blocks' loads in flight together
                const f32x4 a0 = a_ok ? *reinterpret_cast<const f32x4*>(arow + k) : zero;
                const f32x4 b0 = b_ok ? *reinterpret_cast<const f32x4*>(brow + k) : zero;
                const f32x4 a1 = a_ok ? *reinterpret_cast<const f32x4*>(arow + k + 16) : zero;
                const f32x4 b1 = b_ok ? *reinterpret_cast<const f32x4*>(brow + k + 16) : zero;
#pragma unroll
                for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[s], b0[s], acc, 0, 0, 0);
#pragma unroll
                for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[s], b1[s], acc, 0, 0, 0);
            }
            // C/D: column l16, row 4 kk + r
#pragma unroll
            for (int r = 0; r < 4; ++r) P[(4 * kk + r) * ld + t * 16 + l16] = acc[r] * scale;
        }
    }
    __syncthreads();
    // 2. exact softmax statistics of the 16 rows over the W' valid columns: 16 lanes per row (row = threadIdx.x / 16), reduced with xor shuffles
    {
        const int r = threadIdx.x >> 4, q = threadIdx.x & 15;
        float* pr = P + r * ld;
        float m = -INFINITY;
        for (int j = q; j < Ws; j += 16) m = fmaxf(m, pr[j]);
        for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 16));
        float s = 0.f;
        for (int j = q; j < Wt; j += 16) {
            const float e = j < Ws ? expf(pr[j] - m) : 0.f;
            pr[j] = e;
            s += e;
        }
        for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 16);
        if (q == 0) inv[r] = 1.0f / s;
    }
    __syncthreads();
    // 3. F_own[i0 .. i0 + 15][ch] = inv[i] * sum_j P[i][j] V_oth[j][ch]: a wave owns two 16-channel tiles (c is a multiple of 32); lane (l16, kk) of
    //    j-block jb holds j = jb + 4 kk + s in step s (A from LDS as one float4, B as four coalesced 64-byte rows of V)
    const float* vb = oth + c;
    float* fo = F + ((size_t)own_img * Hs + h) * (size_t)Ws * c;
    for (int cp = wave; cp < c / 32; cp += 4) {
        const int ch0 = cp * 32 + l16, ch1 = ch0 + 16;
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        for (int jb = 0; jb < Wt; jb += 16) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(P + l16 * ld + jb + 4 * kk);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int j = jb + 4 * kk + s;
                const float* vr = vb + (size_t)(j < Ws ? j : 0) * 2 * c;
                const float v0 = j < Ws ? vr[ch0] : 0.f, v1 = j < Ws ? vr[ch1] : 0.f;
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], v0, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], v1, acc1, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int il = 4 * kk + r, i = i0 + il;
            if (i < Ws) {
                fo[(size_t)i * c + ch0] = acc0[r] * inv[il];
                fo[(size_t)i * c + ch1] = acc1[r] * inv[il];
            }
        }
    }
}

// out[n][y][x][ch] = x[n][y][x][ch] + s[ch] F[n][sy][sx][ch], s = beta (left views, n < B) / gamma (right views); (sy, sx) is PyTorch's
// `F.interpolate(size=(H, W))` (mode 'nearest') index min(floor(dst * (float)in / out), in - 1) in float arithmetic.  Four channels per thread.
__global__ void __launch_bounds__(256) scam_epilogue_kernel(const float* __restrict__ x, const float* __restrict__ F, const float* __restrict__ beta,
                                                            const float* __restrict__ gamma, float* __restrict__ out, int B, int H, int W, int c,
                                                            int Hs, int Ws) {
    const int c4 = c / 4;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = 2ll * B * H * W * c4;
    if (idx >= total) return;
    const int q = (int)(idx % c4);
    const long long p = idx / c4;
    const int xw = (int)(p % W);
    const int y = (int)((p / W) % H);
    const int n = (int)(p / ((long long)W * H));
    const float sh = (float)Hs / (float)H, sw = (float)Ws / (float)W;
    const int sy = min((int)floorf((float)y * sh), Hs - 1), sx = min((int)floorf((float)xw * sw), Ws - 1);
    const float* sc = n < B ? beta : gamma;
    const f32x4 xv = reinterpret_cast<const f32x4*>(x)[idx];
    const f32x4 fv = reinterpret_cast<const f32x4*>(F + (((size_t)n * Hs + sy) * Ws + sx) * c)[q];
    const f32x4 sv = reinterpret_cast<const f32x4*>(sc)[q];
    f32x4 o;
    o[0] = fv[0] * sv[0] + xv[0];
    o[1] = fv[1] * sv[1] + xv[1];
    o[2] = fv[2] * sv[2] + xv[2];
    o[3] = fv[3] * sv[3] + xv[3];
    reinterpret_cast<f32x4*>(out)[idx] = o;
}

// stereo input: xt, cond [B][2 ic][H][W] -> x0 [2B][Hp + 6][Wp + 6][P], image v B + b = view v of pair b, channels {xt_v - cond_v (ic), cond_v (ic), 0 ..},
// zero border of 3 and zero padding to (Hp, Wp) (the NAFNet's check_image_size)
__global__ void stereo_prep_kernel(const float* __restrict__ xt, const float* __restrict__ cond, float* __restrict__ x0, int B, int ic, int P, int H,
                                   int W, int Hp, int Wp) {
    const int Hb = Hp + 6, Wb = Wp + 6;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 2ll * B * Hb * Wb) return;
    const int xb = (int)(idx % Wb);
    const int yb = (int)((idx / Wb) % Hb);
    const int n = (int)(idx / ((long long)Wb * Hb));
    const int v = n / B, b = n % B;
    const int y = yb - 3, x = xb - 3;
    const bool in = y >= 0 && y < H && x >= 0 && x < W;
    float* o = x0 + idx * P;
    for (int ch = 0; ch < ic; ++ch) {
        float a = 0.f, cv = 0.f;
        if (in) {
            const size_t s = (((size_t)b * 2 * ic + v * ic + ch) * H + y) * W + x;
            cv = cond[s];
            a = xt[s] - cv;
        }
        o[ch] = a;
        o[ic + ch] = cv;
    }
    for (int ch = 2 * ic; ch < P; ++ch) o[ch] = 0.f;
}

// ending output [2B][Hp][Wp][in_stride] -> eps_hat [B][Hp][Wp][out_stride], channel v ic + ch of pair b = channel ch of image v B + b
__global__ void stereo_pack_pred_kernel(const float* __restrict__ in, float* __restrict__ out, int B, int ic, int HWp, int in_stride, int out_stride) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)B * HWp) return;
    const int b = (int)(idx / HWp), p = (int)(idx % HWp);
    for (int v = 0; v < 2; ++v)
        for (int ch = 0; ch < ic; ++ch) out[idx * out_stride + v * ic + ch] = in[((size_t)(v * B + b) * HWp + p) * in_stride + ch];
}


// ---- full-resolution SCAM (stereo-sr ConditionalUNet) ----

// one wave per pixel (n, h, w): x2 = [LN(x) * g | x]; channel ch = lane + 64 q (c <= 2048: q < 32).  module_util.LayerNorm: biased variance, eps 1e-5,
// gain only.
__global__ void __launch_bounds__(256) scam_full_prologue_kernel(const float* __restrict__ x, const float* __restrict__ g_l,
                                                                 const float* __restrict__ g_r, float* __restrict__ x2, long long npix,
                                                                 long long pix_per_view, int c) {
    const int lane = threadIdx.x & 63;
    const long long pix = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pix >= npix) return;
    const float* g = pix < pix_per_view ? g_l : g_r;
    const float* xp = x + (size_t)pix * c;
    float v[32];
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < 32; ++q) {
        const int ch = lane + 64 * q;
        v[q] = ch < c ? xp[ch] : 0.f;
        sum += v[q];
    }
    const float mean = wave_sum(sum) / (float)c;
    float sq = 0.f;
#pragma unroll
    for (int q = 0; q < 32; ++q) {
        const int ch = lane + 64 * q;
        if (ch < c) {
            const float d = v[q] - mean;
            sq += d * d;
        }
    }
    const float rstd = rsqrtf(wave_sum(sq) / (float)c + 1e-5f);
    float* o = x2 + (size_t)pix * 2 * c;
#pragma unroll
    for (int q = 0; q < 32; ++q) {
        const int ch = lane + 64 * q;
        if (ch < c) {
            o[ch] = (v[q] - mean) * rstd * g[ch];
            o[c + ch] = v[q];
        }
    }
}

// grid (strips = ceil(W / 16), B * H, 2 directions), 256 threads.  qv: [2B][H][W][Q (c) | V (c)], F: [2B][H][W][c].
// LDS: P[16][ld] (ld = Wt + 4, Wt = 16 ceil(W / 16)) + inv[16].  NT: column tiles per wave (Wt <= 64 NT).
template <int NT>
__global__ void __launch_bounds__(256) scam_full_core_kernel(const float* __restrict__ qv, float* __restrict__ F, int B, int H, int W, int c,
                                                             float scale) {
    extern __shared__ float lds[];
    const int Wt = (W + 15) & ~15, ld = Wt + 4;
    float* P = lds;
    float* inv = lds + 16 * ld;
    const int strip = blockIdx.x, row = blockIdx.y, dir = blockIdx.z;
    const int b = row / H, h = row % H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l16 = lane & 15, kk = lane >> 4;
    const size_t rowsz = (size_t)W * 2 * c;
    const int own_img = dir == 0 ? b : B + b, oth_img = dir == 0 ? B + b : b;
    const float* own = qv + ((size_t)own_img * H + h) * rowsz;   // strip rows: Q at [0, c)
    const float* oth = qv + ((size_t)oth_img * H + h) * rowsz;   // other view: Q at [0, c), V at [c, 2c)
    const int i0 = strip * 16;
    const int ntile = Wt / 16;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    // 1. S strip [16][Wt] = scale * Q_own[i0 .. i0 + 15] . Q_oth^T: k on the outside, the wave's tiles t = wave + 4 u in accumulators.  Lane (l16, kk)
    //    of k-block kb holds k = kb + 4 kk + s in MFMA step s for both operands (a k permutation shared by A and B leaves the sum unchanged).
    {
        const int ia = i0 + l16;
        const bool a_ok = ia < W;
        const float* arow = own + (size_t)(a_ok ? ia : 0) * 2 * c + 4 * kk;
        f32x4 acc[NT];
#pragma unroll
        for (int u = 0; u < NT; ++u) acc[u] = zero;
        for (int k = 0; k < c; k += 32) {
            const f32x4 a0 = a_ok ? *reinterpret_cast<const f32x4*>(arow + k) : zero;
            const f32x4 a1 = a_ok ? *reinterpret_cast<const f32x4*>(arow + k + 16) : zero;
#pragma unroll
            for (int u = 0; u < NT; ++u) {
                const int t = wave + 4 * u;
                if (t < ntile) {   // (wave-uniform)
                    const int jb = t * 16 + l16;
                    const bool b_ok = jb < W;
                    const float* brow = oth + (size_t)(b_ok ? jb : 0) * 2 * c + 4 * kk + k;
                    const f32x4 b0 = b_ok ? *reinterpret_cast<const f32x4*>(brow) : zero;
                    const f32x4 b1 = b_ok ? *reinterpret_cast<const f32x4*>(brow + 16) : zero;
#pragma unroll
                    for (int s = 0; s < 4; ++s) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[s], b0[s], acc[u], 0, 0, 0);
#pragma unroll
                    for (int s = 0; s < 4; ++s) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[s], b1[s], acc[u], 0, 0, 0);
                }
            }
        }
        // C/D: column l16, row 4 kk + r
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            const int t = wave + 4 * u;
            if (t < ntile) {
#pragma unroll
                for (int r = 0; r < 4; ++r) P[(4 * kk + r) * ld + t * 16 + l16] = acc[u][r] * scale;
            }
        }
    }
    __syncthreads();
    // 2. exact softmax statistics of the 16 rows over the W valid columns: 16 lanes per row, reduced with xor shuffles (two passes: max, then sum)
    {
        const int r = threadIdx.x >> 4, q = threadIdx.x & 15;
        float* pr = P + r * ld;
        float m = -INFINITY;
        for (int j = q; j < W; j += 16) m = fmaxf(m, pr[j]);
        for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 16));
        float s = 0.f;
        for (int j = q; j < Wt; j += 16) {
            const float e = j < W ? expf(pr[j] - m) : 0.f;
            pr[j] = e;
            s += e;
        }
        for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 16);
        if (q == 0) inv[r] = 1.0f / s;
    }
    __syncthreads();
    // 3. F_own[i0 .. i0 + 15][ch] = inv[i] * sum_j P[i][j] V_oth[j][ch]: a wave owns two 16-channel tiles per pass (c is a multiple of 32)
    const float* vb = oth + c;
    float* fo = F + ((size_t)own_img * H + h) * (size_t)W * c;
    for (int cp = wave; cp < c / 32; cp += 4) {
        const int ch0 = cp * 32 + l16, ch1 = ch0 + 16;
        f32x4 acc0 = zero, acc1 = zero;
        for (int jb = 0; jb < Wt; jb += 16) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(P + l16 * ld + jb + 4 * kk);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int j = jb + 4 * kk + s;
                const float* vr = vb + (size_t)(j < W ? j : 0) * 2 * c;
                const float v0 = j < W ? vr[ch0] : 0.f, v1 = j < W ? vr[ch1] : 0.f;
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], v0, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], v1, acc1, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int il = 4 * kk + r, i = i0 + il;
            if (i < W) {
                fo[(size_t)i * c + ch0] = acc0[r] * inv[il];
                fo[(size_t)i * c + ch1] = acc1[r] * inv[il];
            }
        }
    }
}

// x[n][y][x][ch] += s[ch] F[n][y][x][ch] in place, s = beta (left views) / gamma (right views).  Four channels per thread.
__global__ void __launch_bounds__(256) scam_full_epilogue_kernel(float* __restrict__ x, const float* __restrict__ F, const float* __restrict__ beta,
                                                                 const float* __restrict__ gamma, long long total, long long quads_per_view, int c4) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int q = (int)(idx % c4);
    const float* sc = idx < quads_per_view ? beta : gamma;
    const f32x4 xv = reinterpret_cast<const f32x4*>(x)[idx];
    const f32x4 fv = reinterpret_cast<const f32x4*>(F)[idx];
    const f32x4 sv = reinterpret_cast<const f32x4*>(sc)[q];
    f32x4 o;
    o[0] = fv[0] * sv[0] + xv[0];
    o[1] = fv[1] * sv[1] + xv[1];
    o[2] = fv[2] * sv[2] + xv[2];
    o[3] = fv[3] * sv[3] + xv[3];
    reinterpret_cast<f32x4*>(x)[idx] = o;
}

// stereo UNet input: xt, cond [B][2 ic][H][W] -> x0 [2B][Hp + 6][Wp + 6][P], image v B + b = view v of pair b, channels {xt_v (ic), cond_v (ic), 0 ..}
// (no xt - cond: stereo-sr DenoisingUNet_arch.py:143-147), F.pad 'reflect' to (Hp, Wp) and a zero border of 3
__global__ void stereo_unet_prep_kernel(const float* __restrict__ xt, const float* __restrict__ cond, float* __restrict__ x0, int B, int ic, int P,
                                        int H, int W, int Hp, int Wp) {
    const int Hb = Hp + 6, Wb = Wp + 6;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 2ll * B * Hb * Wb) return;
    const int xb = (int)(idx % Wb);
    const int yb = (int)((idx / Wb) % Hb);
    const int n = (int)(idx / ((long long)Wb * Hb));
    const int v = n / B, b = n % B;
    const int y = yb - 3, x = xb - 3;
    const bool in = y >= 0 && y < Hp && x >= 0 && x < Wp;
    const int sy = y < H ? y : 2 * (H - 1) - y, sx = x < W ? x : 2 * (W - 1) - x;
    float* o = x0 + idx * P;
    for (int ch = 0; ch < ic; ++ch) {
        float a = 0.f, cv = 0.f;
        if (in) {
            const size_t s = (((size_t)b * 2 * ic + v * ic + ch) * H + sy) * W + sx;
            cv = cond[s];
            a = xt[s];
        }
        o[ch] = a;
        o[ic + ch] = cv;
    }
    for (int ch = 2 * ic; ch < P; ++ch) o[ch] = 0.f;
}

// final_conv output [2B][Hp][Wp][in_stride] + the pair state xt [B][2 ic][H][W] -> eps_hat [B][Hp][Wp][out_stride]:
// channel v ic + ch of pair b = xt[b][v ic + ch] + channel ch of image v B + b (xt_res + cat(x_l, x_r), :193-194; nothing is added in the padding)
__global__ void stereo_unet_pack_pred_kernel(const float* __restrict__ in, const float* __restrict__ xt, float* __restrict__ out, int B, int ic, int H,
                                             int W, int Hp, int Wp, int in_stride, int out_stride) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int HWp = Hp * Wp;
    if (idx >= (long long)B * HWp) return;
    const int b = (int)(idx / HWp), p = (int)(idx % HWp);
    const int y = p / Wp, x = p % Wp;
    const bool inside = y < H && x < W;
    for (int v = 0; v < 2; ++v)
        for (int ch = 0; ch < ic; ++ch) {
            const float r = inside ? xt[(((size_t)b * 2 * ic + v * ic + ch) * H + y) * W + x] : 0.f;
            out[idx * out_stride + v * ic + ch] = r + in[((size_t)(v * B + b) * HWp + p) * in_stride + ch];
        }
}

}  // namespace

void scam_full_check_shape(int H, int W, int c, bool any_width) {
    if (H < 1 || W < 1) throw HipError("SCAM (full resolution): empty feature map");
    if (c % 32 || c < 32 || c > kScamFullMaxC) throw HipError("SCAM (full resolution): channel count must be a multiple of 32 in [32, 2048]");
    if (W > kScamFullMaxW && !any_width)
        throw HipError("SCAM (full resolution): feature maps wider than 1024 pixels are not supported (the 16 x W score strip must fit LDS; "
                       "IRSDE_FLAG_SCAM_STREAM runs them on the streaming core)");
}

void launch_scam_full_prologue(const float* x, const float* g_l, const float* g_r, float* x2, int B, int H, int W, int c, hipStream_t s) {
    const long long per_view = (long long)B * H * W, npix = 2 * per_view;
    hipLaunchKernelGGL(scam_full_prologue_kernel, dim3((unsigned)((npix + 3) / 4)), dim3(256), 0, s, x, g_l, g_r, x2, npix, per_view, c);
    IRSDE_HIP_CHECK(hipGetLastError());
}

void launch_scam_full_core(const float* qv, float* F, int B, int H, int W, int c, hipStream_t s) {
    scam_full_check_shape(H, W, c);
    if ((long long)B * H > 65535) throw HipError("SCAM (full resolution): more than 65535 image rows in one launch");
    const int Wt = (W + 15) & ~15;
    const size_t lds = (size_t)(16 * (Wt + 4) + 16) * sizeof(float);
    const dim3 grid((unsigned)(Wt / 16), (unsigned)(B * H), 2);
    const float scale = 1.0f / sqrtf((float)c);
    if (Wt <= 256) {
        hipLaunchKernelGGL(scam_full_core_kernel<4>, grid, dim3(256), lds, s, qv, F, B, H, W, c, scale);
    } else if (Wt <= 512) {
        hipLaunchKernelGGL(scam_full_core_kernel<8>, grid, dim3(256), lds, s, qv, F, B, H, W, c, scale);
    } else {
        // up to 66 KB of dynamic LDS: above the 64 KB default (per device, so set at every launch: a host-side call, legal during capture)
        IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&scam_full_core_kernel<16>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)((16 * (kScamFullMaxW + 4) + 16) * sizeof(float))));
        hipLaunchKernelGGL(scam_full_core_kernel<16>, grid, dim3(256), lds, s, qv, F, B, H, W, c, scale);
    }
    IRSDE_HIP_CHECK(hipGetLastError());
}

void launch_scam_full_epilogue(float* x, const float* F, const float* beta, const float* gamma, int B, int H, int W, int c, hipStream_t s) {
    const long long per_view = (long long)B * H * W * (c / 4), total = 2 * per_view;
    hipLaunchKernelGGL(scam_full_epilogue_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, F, beta, gamma, total, per_view, c / 4);
    IRSDE_HIP_CHECK(hipGetLastError());
}

void launch_stereo_unet_prep(const float* xt, const float* cond, float* x0, int B, int ic, int P, int H, int W, int Hp, int Wp, hipStream_t s) {
    const long long total = 2ll * B * (Hp + 6) * (Wp + 6);
    hipLaunchKernelGGL(stereo_unet_prep_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, xt, cond, x0, B, ic, P, H, W, Hp, Wp);
    IRSDE_HIP_CHECK(hipGetLastError());
}

void launch_stereo_unet_pack_pred(const float* in, const float* xt, float* out, int B, int ic, int H, int W, int Hp, int Wp, int in_stride,
                                  int out_stride, hipStream_t s) {
    const long long total = (long long)B * Hp * Wp;
    hipLaunchKernelGGL(stereo_unet_pack_pred_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, in, xt, out, B, ic, H, W, Hp, Wp, in_stride,
                       out_stride);
    IRSDE_HIP_CHECK(hipGetLastError());
}

void scam_check_shape(int H, int W, int c, bool any_width) {
    if (H < 4 || W < 4) throw HipError("SCAM: the feature map must have at least 4 rows and columns (the bicubic quarter-downsample of the reference "
                                       "is empty below that): pad the stereo input to a larger size");
    if (c % 32 || c < 32 || c > 1024) throw HipError("SCAM: channel count must be a multiple of 32 in [32, 1024]");
    if (W / 4 > kScamMaxWs && !any_width)
        throw HipError("SCAM: feature maps wider than 2051 pixels are not supported (W / 4 <= 512; IRSDE_FLAG_SCAM_STREAM runs them on the streaming core)");
}

void launch_scam_prologue(const float* x, const float* g_l, const float* g_r, float* xs2, int B, int H, int W, int c, hipStream_t s) {
    const int Hs = H / 4, Ws = W / 4;
    const long long npix = 2ll * B * Hs * Ws;
    hipLaunchKernelGGL(scam_prologue_kernel, dim3((unsigned)((npix + 3) / 4)), dim3(256), 0, s, x, g_l, g_r, xs2, B, H, W, c, Hs, Ws);
    IRSDE_HIP_CHECK(hipGetLastError());
}

void launch_scam_core(const float* qv, float* F, int B, int H, int W, int c, hipStream_t s) {
    const int Hs = H / 4, Ws = W / 4;
    const int Wt = (Ws + 15) & ~15;
    const size_t lds = (size_t)(16 * (Wt + 4) + 16) * sizeof(float);
    hipLaunchKernelGGL(scam_core_kernel, dim3((unsigned)(Wt / 16), (unsigned)(B * Hs), 2), dim3(256), lds, s, qv, F, B, Hs, Ws, c,
                       1.0f / sqrtf((float)c));
    IRSDE_HIP_CHECK(hipGetLastError());
}

void launch_scam_epilogue(const float* x, const float* F, const float* beta, const float* gamma, float* out, int B, int H, int W, int c, hipStream_t s) {
    const long long total = 2ll * B * H * W * (c / 4);
    hipLaunchKernelGGL(scam_epilogue_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, F, beta, gamma, out, B, H, W, c, H / 4, W / 4);
    IRSDE_HIP_CHECK(hipGetLastError());
}

void launch_stereo_prep(const float* xt, const float* cond, float* x0, int B, int ic, int P, int H, int W, int Hp, int Wp, hipStream_t s) {
    const long long total = 2ll * B * (Hp + 6) * (Wp + 6);
    hipLaunchKernelGGL(stereo_prep_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, xt, cond, x0, B, ic, P, H, W, Hp, Wp);
    IRSDE_HIP_CHECK(hipGetLastError());
}

void launch_stereo_pack_pred(const float* in, float* out, int B, int ic, int Hp, int Wp, int in_stride, int out_stride, hipStream_t s) {
    const long long total = (long long)B * Hp * Wp;
    hipLaunchKernelGGL(stereo_pack_pred_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, in, out, B, ic, Hp * Wp, in_stride, out_stride);
    IRSDE_HIP_CHECK(hipGetLastError());
}

// [[w1, 0], [0, w2]] ([2c][2c], 1x1 kernel layout [Cout][Cin]) and [b1 | b2] from reference-layout [c][c] weights
void scam_pack_proj(const float* w1, const float* b1, const float* w2, const float* b2, int c, std::vector<float>& w, std::vector<float>& bias) {
    w.assign((size_t)4 * c * c, 0.f);
    bias.resize(2 * (size_t)c);
    for (int o = 0; o < c; ++o) {
        for (int k = 0; k < c; ++k) {
            w[(size_t)o * 2 * c + k] = w1[(size_t)o * c + k];
            w[(size_t)(c + o) * 2 * c + c + k] = w2[(size_t)o * c + k];
        }
        bias[o] = b1[o];
        bias[c + o] = b2[o];
    }
}

}  // namespace irsde
