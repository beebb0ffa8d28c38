// Degradation front ends of the reference's test loops on the device (codes/utils/deg_utils.py):
//   upscale  (:38-40)  F.interpolate(x, scale_factor=s, mode='bicubic') for integer s — sisr/test.py:102, stereo-sr/test.py:105-109
//   mask_to  (:19-34)  mask * x + (1 - mask) with the uint8 mask / 255. resized by nearest interpolation — inpainting/test.py:103
// Both are streaming kernels on NCHW fp32: the upscale writes s^2 times what it reads, the composite reads and writes one float per element.
// This file is compiled with -ffp-contract=off: the composite keeps the reference's multiply / subtract / add as three roundings.  The
// upscale's filter sums are explicit fmaf chains (its contract is the 1e-5 parity with the float64 restatement, not an op order).
//   imresize (codes/data/util.py:238-387)  the antialiased cubic downscale that makes LQ from GT (LQGT_dataset.py:106-130): one table-driven
//   kernel, H pass into LDS, W pass out; explicit fmaf chains in tap order as well.
#include "common.h"

namespace irsde {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------
// Bicubic upscale, align_corners=False, A = -0.75.  Output index o samples the input at src = (o + 0.5) / S - 0.5 =
// (2 o + 1 - S) / (2 S): with o = S i + p (p = o mod S) the integer part is i0 = i + d(p), d(p) = -1 where 2 p + 1 < S and 0
// otherwise, and the fraction t(p) = ((2 p + 1 - S) mod 2 S) / (2 S) depends on p alone — all in exact integer arithmetic.  The four
// taps i0 - 1 .. i0 + 2 are clamped to the image; src is not.  One S x 4 table serves both axes (the scale is the same).
//
// A work-group owns IH x UP_IW input pixels = (IH S) x (UP_IW S) outputs of one plane (IH = up_ih(S): 16 rows for S <= 2, 4 for S >= 6, else 8,
// so a work-group writes 8 - 32 KB at every factor):
//   1. the clamped (IH + 4) x (UP_IW + 4) input patch -> LDS (rows / columns i - 2 .. i + 2 around the tile: d(p) = -1 reaches i - 2)
//   2. horizontal pass: (IH + 4) rows x UP_IW S columns -> LDS
//   3. vertical pass from LDS: a lane forms 4 neighbouring outputs of a row from four 16-byte LDS reads and stores them as one
//      16-byte piece (rows whose length or base address is no multiple of 4 floats, e.g. S = 3 on an odd width, take the
//      element-per-lane path: consecutive lanes, consecutive floats).
// ---------------------------------------------------------------------------------------------
constexpr int UP_IW = 32, UP_THREADS = 256;
constexpr int up_ih(int S) { return S <= 2 ? 16 : (S >= 6 ? 4 : 8); }

template <int S>
__global__ void __launch_bounds__(UP_THREADS) upscale_bicubic_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W,
                                                                     int tiles_x, int tiles_y, int vec) {
    constexpr int IH = up_ih(S), PH = IH + 4, PW = UP_IW + 4, TW = UP_IW * S, TH = IH * S;
    __shared__ float wtab[S][4];
    __shared__ int dtab[S];
    __shared__ float patch[PH][PW];
    __shared__ __attribute__((aligned(16))) float hrow[PH][TW];
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % tiles_x;
    const int ty = (blockIdx.x / tiles_x) % tiles_y;
    const size_t plane = blockIdx.x / ((size_t)tiles_x * tiles_y);
    const int iy0 = ty * IH, ix0 = tx * UP_IW;
    const float* src = in + plane * (size_t)H * W;
    const int Ho = H * S, Wo = W * S;
    float* dst = out + plane * (size_t)Ho * Wo;

    if (tid < S) {
        const int num = 2 * tid + 1 - S;                       // (2 p + 1 - S), in (-S, S)
        const int d = num < 0 ? -1 : 0;
        const double A = -0.75, t = (double)(num - d * 2 * S) / (double)(2 * S);
        const double x0 = t + 1.0, x1 = t, x2 = 1.0 - t, x3 = 2.0 - t;
        wtab[tid][0] = (float)(((A * x0 - 5.0 * A) * x0 + 8.0 * A) * x0 - 4.0 * A);
        wtab[tid][1] = (float)(((A + 2.0) * x1 - (A + 3.0)) * x1 * x1 + 1.0);
        wtab[tid][2] = (float)(((A + 2.0) * x2 - (A + 3.0)) * x2 * x2 + 1.0);
        wtab[tid][3] = (float)(((A * x3 - 5.0 * A) * x3 + 8.0 * A) * x3 - 4.0 * A);
        dtab[tid] = d;
    }
    for (int e = tid; e < PH * PW; e += UP_THREADS) {
        const int r = e / PW, c = e - r * PW;
        const int y = min(max(iy0 - 2 + r, 0), H - 1), x = min(max(ix0 - 2 + c, 0), W - 1);
        patch[r][c] = src[(size_t)y * W + x];
    }
    __syncthreads();
    for (int e = tid; e < PH * TW; e += UP_THREADS) {
        const int r = e / TW, xo = e - r * TW;
        const int p = xo % S;
        const float* q = &patch[r][xo / S + dtab[p] + 1];        // patch column of tap i0 - 1
        float a = wtab[p][0] * q[0];
        a = fmaf(wtab[p][1], q[1], a);
        a = fmaf(wtab[p][2], q[2], a);
        a = fmaf(wtab[p][3], q[3], a);
        hrow[r][xo] = a;
    }
    __syncthreads();
    const int oy0 = iy0 * S, ox0 = ix0 * S;
    if (vec) {
        constexpr int GW = TW / 4;   // 16-byte pieces per tile row
        for (int g = tid; g < TH * GW; g += UP_THREADS) {
            const int yo = g / GW, xg = (g - yo * GW) * 4;
            const int oy = oy0 + yo, ox = ox0 + xg;
            if (oy >= Ho || ox >= Wo) continue;                  // Wo % 4 == 0 here: a piece never straddles the edge
            const int p = yo % S, r = yo / S + dtab[p] + 1;
            const float w0 = wtab[p][0], w1 = wtab[p][1], w2 = wtab[p][2], w3 = wtab[p][3];
            const f32x4 v0 = *reinterpret_cast<const f32x4*>(&hrow[r][xg]);
            const f32x4 v1 = *reinterpret_cast<const f32x4*>(&hrow[r + 1][xg]);
            const f32x4 v2 = *reinterpret_cast<const f32x4*>(&hrow[r + 2][xg]);
            const f32x4 v3 = *reinterpret_cast<const f32x4*>(&hrow[r + 3][xg]);
            f32x4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = fmaf(w3, v3[k], fmaf(w2, v2[k], fmaf(w1, v1[k], w0 * v0[k])));
            *reinterpret_cast<f32x4*>(dst + (size_t)oy * Wo + ox) = o;
        }
    } else {
        for (int e = tid; e < TH * TW; e += UP_THREADS) {
            const int yo = e / TW, xo = e - yo * TW;
            const int oy = oy0 + yo, ox = ox0 + xo;
            if (oy >= Ho || ox >= Wo) continue;
            const int p = yo % S, r = yo / S + dtab[p] + 1;
            dst[(size_t)oy * Wo + ox] =
                fmaf(wtab[p][3], hrow[r + 3][xo], fmaf(wtab[p][2], hrow[r + 2][xo], fmaf(wtab[p][1], hrow[r + 1][xo], wtab[p][0] * hrow[r][xo])));
        }
    }
}

template <int S>
void launch_upscale(const float* in, float* out, size_t planes, int H, int W, hipStream_t s) {
    const int tiles_x = (W + UP_IW - 1) / UP_IW, tiles_y = (H + up_ih(S) - 1) / up_ih(S);
    const size_t blocks = planes * tiles_x * tiles_y;
    if (blocks > 0x7fffffffull) throw HipError("upscale_bicubic: too many tiles for one launch");
    const int vec = ((W * S) % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) ? 1 : 0;
    hipLaunchKernelGGL(upscale_bicubic_kernel<S>, dim3((unsigned)blocks), dim3(UP_THREADS), 0, s, in, out, H, W, tiles_x, tiles_y, vec);
    IRSDE_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------
// out = mask * x + (1 - mask), mask[b][c][y][x] = (float)((double)m8[bm][sy][sx][cm] / 255.0), (sy, sx) PyTorch's nearest index
// min(floor(dst * (float)in / out), in - 1) in float arithmetic (as scam_epilogue_kernel).  A lane owns up to 4 neighbouring
// elements of a row; `vec`: W % 4 == 0 and 16-byte aligned tensors, one 16-byte load and store per lane.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float mask_composite(float x, unsigned char m8) {
    const float m = (float)((double)m8 / 255.0);
    const float mx = m * x;          // masked_tensor = mask * tensor
    const float om = 1.0f - m;       // (1. - mask)
    return mx + om;
}

__global__ void __launch_bounds__(256) mask_to_kernel(const float* __restrict__ x, const unsigned char* __restrict__ m8, int Bm, int Hm, int Wm,
                                                      int Cm, float* __restrict__ out, int B, int C, int H, int W, int vec) {
    const int W4 = (W + 3) / 4;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)B * C * H * W4;
    if (idx >= total) return;
    const int xq = (int)(idx % W4) * 4;
    const size_t row = idx / W4;                 // (b C + c) H + y
    const int y = (int)(row % H);
    const size_t pc = row / H;
    const int c = (int)(pc % C), b = (int)(pc / C);
    const float sh = (float)Hm / (float)H, sw = (float)Wm / (float)W;
    const int sy = min((int)floorf((float)y * sh), Hm - 1);
    const unsigned char* mrow = m8 + (((size_t)(Bm == 1 ? 0 : b) * Hm + sy) * Wm) * Cm + (Cm == 1 ? 0 : c);
    const size_t base = row * W + xq;
    if (vec) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + base);
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int sx = min((int)floorf((float)(xq + k) * sw), Wm - 1);
            o[k] = mask_composite(xv[k], mrow[(size_t)sx * Cm]);
        }
        *reinterpret_cast<f32x4*>(out + base) = o;
    } else {
        for (int k = 0; k < 4 && xq + k < W; ++k) {
            const int sx = min((int)floorf((float)(xq + k) * sw), Wm - 1);
            out[base + k] = mask_composite(x[base + k], mrow[(size_t)sx * Cm]);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// imresize (codes/data/util.py:305-387), the MATLAB-style separable cubic resize that makes LQ from GT.  Table-driven: the host builds, per
// axis, weights w[n_out][K] and the 0-based image coordinate start[n_out] of each output's first tap (degradations.imresize_tables, the
// reference's own float32 values), so one kernel serves every scale and both antialiasing settings.  A tap at p < 0 reads pixel -p - 1, a
// tap at p >= n reads 2 n - 1 - p: the reference's symmetric border copies, taken in place.
//
// A work-group owns TY x IMR_TX outputs of one plane.  As in the reference the H axis is filtered first: for the tile's TY output rows
// and the columns [sW[x0], sW[x1 - 1] + KW) its W filters reach (the start table is non-decreasing), lanes on consecutive columns sum KH
// rows of the input into LDS — the reference's out_1, which never reaches memory; a reflected column of out_1 is the H filter of the
// reflected input column, bit for bit.  The W pass then sums KW neighbours of an LDS row per output.  Every sum is w[0] v[0] followed by
// fmaf in tap order; the values of four taps are fetched before their four fmaf, so that four loads are in flight, not one.
// ---------------------------------------------------------------------------------------------
constexpr int IMR_THREADS = 256, IMR_TX = 32, IMR_TY = 16, IMR_TAPS = 32, IMR_MID = 4608;   // LDS: 18 KB of H-pass rows + 6.3 KB of tables

__device__ __forceinline__ int imr_reflect(int p, int n) {
    p = p < 0 ? -p - 1 : p;
    p = p >= n ? 2 * n - 1 - p : p;
    return min(max(p, 0), n - 1);   // no table that imresize_tables accepts reaches this clamp; it keeps any other table inside the plane
}

// w[0] ld(0), then fmaf(w[k], ld(k), .) for k = 1 .. K - 1
template <class Ld>
__device__ __forceinline__ float imr_sum(const float* w, int K, Ld ld) {
    float a;
    int k;
    if (K >= 4) {
        const float v0 = ld(0), v1 = ld(1), v2 = ld(2), v3 = ld(3);
        a = fmaf(w[3], v3, fmaf(w[2], v2, fmaf(w[1], v1, w[0] * v0)));
        k = 4;
    } else {
        a = w[0] * ld(0);
        k = 1;
    }
    for (; k + 4 <= K; k += 4) {
        const float v0 = ld(k), v1 = ld(k + 1), v2 = ld(k + 2), v3 = ld(k + 3);
        a = fmaf(w[k + 3], v3, fmaf(w[k + 2], v2, fmaf(w[k + 1], v1, fmaf(w[k], v0, a))));
    }
    for (; k < K; ++k) a = fmaf(w[k], ld(k), a);
    return a;
}

__global__ void __launch_bounds__(IMR_THREADS) imresize_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int Ho, int Wo,
                                                               const float* __restrict__ wH, const int* __restrict__ sH, int KH,
                                                               const float* __restrict__ wW, const int* __restrict__ sW, int KW, int TY,
                                                               int tiles_x, int tiles_y, int vec) {
    __shared__ __attribute__((aligned(16))) float wHs[IMR_TY][IMR_TAPS];
    __shared__ float wWs[IMR_TX][IMR_TAPS + 1];   // + 1: lanes of the W pass read one column of different rows
    __shared__ int sHs[IMR_TY], sWs[IMR_TX];
    __shared__ float mid[IMR_MID];
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % tiles_x;
    const int ty = (blockIdx.x / tiles_x) % tiles_y;
    const size_t plane = blockIdx.x / ((size_t)tiles_x * tiles_y);
    const int y0 = ty * TY, x0 = tx * IMR_TX;
    const int ny = min(TY, Ho - y0), nx = min(IMR_TX, Wo - x0);
    const float* src = in + plane * (size_t)H * W;
    float* dst = out + plane * (size_t)Ho * Wo;

    for (int e = tid; e < ny * KH; e += IMR_THREADS) {
        const int r = e / KH, k = e - r * KH;
        wHs[r][k] = wH[(size_t)(y0 + r) * KH + k];
    }
    for (int e = tid; e < nx * KW; e += IMR_THREADS) {
        const int j = e / KW, l = e - j * KW;
        wWs[j][l] = wW[(size_t)(x0 + j) * KW + l];
    }
    if (tid < ny) sHs[tid] = sH[y0 + tid];
    if (tid < nx) sWs[tid] = sW[x0 + tid];
    __syncthreads();
    const int c0 = sWs[0];
    const long long span64 = (long long)sWs[nx - 1] + KW - c0;
    // the launcher sizes TY so that the tile's rows fit; a start table that decreases or jumps is not one of imresize_tables', and the whole
    // group leaves before it could index past `mid`
    if (span64 < KW || ny * span64 > IMR_MID) return;
    const int span = (int)span64;
    for (int e = tid; e < ny * span; e += IMR_THREADS) {
        const int r = e / span, c = e - r * span;
        const float* col = src + imr_reflect(c0 + c, W);
        const int ys = sHs[r];
        float a;
        if (ys >= 0 && ys <= H - KH) {                          // every tap inside the image: rows ys .. ys + KH - 1
            const float* p = col + (size_t)ys * W;
            a = imr_sum(wHs[r], KH, [&](int k) { return p[(size_t)k * W]; });
        } else {
            a = imr_sum(wHs[r], KH, [&](int k) { return col[(size_t)imr_reflect(ys + k, H) * W]; });
        }
        mid[e] = a;                                             // mid[r][c], rows of `span` floats
    }
    __syncthreads();
    if (vec) {
        constexpr int GW = IMR_TX / 4;   // 16-byte pieces per tile row
        for (int g = tid; g < ny * GW; g += IMR_THREADS) {
            const int r = g / GW, j4 = (g - r * GW) * 4;
            if (j4 >= nx) continue;                             // Wo % 4 == 0 here: a piece never straddles the edge
            f32x4 o;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float* m = mid + r * span + min(max(sWs[j4 + q] - c0, 0), span - KW);
                o[q] = imr_sum(wWs[j4 + q], KW, [&](int l) { return m[l]; });
            }
            *reinterpret_cast<f32x4*>(dst + (size_t)(y0 + r) * Wo + x0 + j4) = o;
        }
    } else {
        for (int e = tid; e < ny * IMR_TX; e += IMR_THREADS) {
            const int r = e / IMR_TX, j = e - r * IMR_TX;
            if (j >= nx) continue;
            const float* m = mid + r * span + min(max(sWs[j] - c0, 0), span - KW);
            dst[(size_t)(y0 + r) * Wo + x0 + j] = imr_sum(wWs[j], KW, [&](int l) { return m[l]; });
        }
    }
}

}  // namespace

void upscale_bicubic(const float* in, float* out, int B, int C, int H, int W, int scale, hipStream_t s) {
    const size_t planes = (size_t)B * C;
    if (scale == 1) {   // t = 0: the filter is the identity (weights 0, 1, 0, 0); a copy keeps every bit pattern
        IRSDE_HIP_CHECK(hipMemcpyAsync(out, in, planes * H * W * sizeof(float), hipMemcpyDeviceToDevice, s));
        return;
    }
    switch (scale) {
        case 2: launch_upscale<2>(in, out, planes, H, W, s); break;
        case 3: launch_upscale<3>(in, out, planes, H, W, s); break;
        case 4: launch_upscale<4>(in, out, planes, H, W, s); break;
        case 5: launch_upscale<5>(in, out, planes, H, W, s); break;
        case 6: launch_upscale<6>(in, out, planes, H, W, s); break;
        case 7: launch_upscale<7>(in, out, planes, H, W, s); break;
        case 8: launch_upscale<8>(in, out, planes, H, W, s); break;
        default: throw HipError("upscale_bicubic: scale must be an integer in 1..8");
    }
}

void mask_to(const float* x, const unsigned char* masks, int Bm, int Hm, int Wm, int Cm, float* out, int B, int C, int H, int W, hipStream_t s) {
    const size_t total = (size_t)B * C * H * ((W + 3) / 4);
    const size_t blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffull) throw HipError("mask_to: too many elements for one launch");
    const int vec = (W % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) == 0) ? 1 : 0;
    hipLaunchKernelGGL(mask_to_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, masks, Bm, Hm, Wm, Cm, out, B, C, H, W, vec);
    IRSDE_HIP_CHECK(hipGetLastError());
}

void imresize(const float* in, float* out, int B, int C, int H, int W, int Ho, int Wo, const float* wH, const int* sH, int KH, const float* wW,
              const int* sW, int KW, hipStream_t s) {
    if (KH < 1 || KH > IMR_TAPS || KW < 1 || KW > IMR_TAPS) throw HipError("imresize: taps per output must be in 1..32");
    // Columns the H pass of a tile covers: its nx outputs' centres lie (nx - 1) / scale apart and Wo = ceil(W scale) gives 1 / scale < W / (Wo - 1);
    // the floor of the start adds at most one, the last output's own taps KW.  At K = 32 (scale 1/8) this is up to 290 columns: 15 rows of them.
    const int nx = Wo < IMR_TX ? Wo : IMR_TX;
    const long long span = (nx > 1 ? ((long long)(nx - 1) * W + Wo - 2) / (Wo - 1) : 0) + KW + 1;
    if (span > IMR_MID) throw HipError("imresize: Wo is too small for W (one row of a tile's H pass does not fit the LDS rows)");
    const int fit = (int)(IMR_MID / span);
    const int TY = fit < IMR_TY ? fit : IMR_TY;
    const int tiles_x = (Wo + IMR_TX - 1) / IMR_TX, tiles_y = (Ho + TY - 1) / TY;
    const size_t blocks = (size_t)B * C * tiles_x * tiles_y;
    if (blocks > 0x7fffffffull) throw HipError("imresize: too many tiles for one launch");
    const int vec = (Wo % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) ? 1 : 0;
    hipLaunchKernelGGL(imresize_kernel, dim3((unsigned)blocks), dim3(IMR_THREADS), 0, s, in, out, H, W, Ho, Wo, wH, sH, KH, wW, sW, KW, TY, tiles_x,
                       tiles_y, vec);
    IRSDE_HIP_CHECK(hipGetLastError());
}

}  // namespace irsde
