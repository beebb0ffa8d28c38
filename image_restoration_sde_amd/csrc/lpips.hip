// LPIPS v0.1, net = 'alex', on the device: the third metric of the reference's test loops (codes/config/deraining/test.py:74, 149-154:
// lpips_fn(GT * 2 - 1, SR * 2 - 1)).  The pip package `lpips` is not part of the reference tree; what it computes is
//   x = (x - shift) / scale per channel; AlexNet `features` tapped after each of its five ReLUs;
//   per tap: n = f / (sqrt(sum_c f^2) + 1e-10), d = (n0 - n1)^2, term = mean over pixels of sum_c w[c] d[c]; lpips = sum of the five terms.
// All of it in fp32:
//   lpips_prologue_kernel   NCHW [-1,1] (or [0,1] with normalize) -> scaled NHWC with 4 channels (the 4th is zero)
//   lpips_conv_kernel       implicit GEMM on v_mfma_f32_32x32x2_f32, bias + ReLU epilogue; one kernel for all five layers (runtime KH / KW / stride / pad)
//   lpips_maxpool_kernel    3x3 stride 2, floor mode, NHWC
//   lpips_dist_kernel       per pixel: two channel norms, the squared difference, the dot with the lin weights; per-block partial sums in a fixed
//                           order (no atomics => deterministic); the host adds the few partials per image in float64 (as eval_metrics.hip does).
// Every output element of a convolution is one fmaf chain over k = (ky, kx, ci) in ascending order, whatever tile it falls into (out-of-image taps and the
// K tail contribute fma(0, w, acc) = acc), so an image's features do not depend on its position in the batch or on the batch size.
#include "common.h"

namespace irsde {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kBM = 64, kBN = 64, kBK = 16;   // block tile: 64 pixels x 64 output channels, 16 k per step; 4 waves, one 32 x 32 MFMA tile each
constexpr int kLD = 68;                       // LDS row pitch in floats (272 bytes: float4-aligned, rows 4 banks apart)

// in0 / in1: NCHW [B][3][H][W]; out: NHWC [2B | B][H][W][4], images [in0_0 .. in0_{B-1}, in1_0 .. in1_{B-1}] (in1 == nullptr: the first B only)
__global__ void lpips_prologue_kernel(const float* __restrict__ in0, const float* __restrict__ in1, float* __restrict__ out, int B, int HW, int N,
                                      int normalize) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)N * HW) return;
    const int n = (int)(i / HW);
    const int pix = (int)(i - (size_t)n * HW);
    const float* src = (n < B ? in0 + (size_t)n * 3 * HW : in1 + (size_t)(n - B) * 3 * HW) + pix;
    const float shift[3] = {-.030f, -.088f, -.188f}, scale[3] = {.458f, .448f, .450f};
    float v[4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float x = src[(size_t)c * HW];
        if (normalize) x = 2.0f * x - 1.0f;
        v[c] = (x - shift[c]) / scale[c];
    }
    v[3] = 0.0f;
    *reinterpret_cast<float4*>(out + i * 4) = make_float4(v[0], v[1], v[2], v[3]);
}

struct LpipsConvArgs {
    const float* in;    // NHWC [N][Hin][Win][Cin], Cin % 4 == 0
    const float* w;     // K-major [K = KH * KW * Cin][Cout], k = (ky * KW + kx) * Cin + ci
    const float* bias;  // [Cout]
    float* out;         // NHWC [N][Ho][Wo][Cout]
    int Hin, Win, Cin, Ho, Wo, Cout, KH, KW, stride, pad, K;
    long long M;        // N * Ho * Wo
};

__global__ __launch_bounds__(256) void lpips_conv_kernel(const LpipsConvArgs a) {
    __shared__ __attribute__((aligned(16))) float As[kBK][kLD];   // [k][pixel]
    __shared__ __attribute__((aligned(16))) float Bs[kBK][kLD];   // [k][cout]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long m0 = (long long)blockIdx.x * kBM;
    const int n0 = blockIdx.y * kBN;

    // A staging: thread -> (pixel am, 4 consecutive k at akq * 4: one tap, 4 consecutive input channels since Cin % 4 == 0)
    const int am = tid >> 2, akq = tid & 3;
    const long long m = m0 + am;
    const bool m_ok = m < a.M;
    int iy0 = 0, ix0 = 0;
    const float* img = a.in;
    if (m_ok) {
        const long long hw = (long long)a.Ho * a.Wo;
        const long long n = m / hw;
        const int r = (int)(m - n * hw);
        const int oy = r / a.Wo, ox = r - oy * a.Wo;
        iy0 = oy * a.stride - a.pad;
        ix0 = ox * a.stride - a.pad;
        img = a.in + (size_t)n * a.Hin * a.Win * a.Cin;
    }
    // B staging: thread -> (k row bk, 4 consecutive couts at bn4 * 4)
    const int bk = tid >> 4, bn4 = tid & 15;
    const bool bn_ok = n0 + bn4 * 4 < a.Cout;   // Cout % 4 == 0

    auto load_a = [&](int kc) {
        const int k = kc + akq * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (m_ok && k < a.K) {
            const int tap = k / a.Cin, ci = k - tap * a.Cin;
            const int ky = tap / a.KW, kx = tap - ky * a.KW;
            const int iy = iy0 + ky, ix = ix0 + kx;
            if (iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win) v = *reinterpret_cast<const float4*>(img + ((size_t)iy * a.Win + ix) * a.Cin + ci);
        }
        return v;
    };
    auto load_b = [&](int kc) {
        const int k = kc + bk;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (bn_ok && k < a.K) v = *reinterpret_cast<const float4*>(a.w + (size_t)k * a.Cout + n0 + bn4 * 4);
        return v;
    };

    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;   // the wave's 32 x 32 tile inside the block tile
    const int fr = lane & 31, fk = lane >> 5;                 // MFMA operand lane map: A[row fr][k fk], B[k fk][col fr]

    float4 ra = load_a(0), rb = load_b(0);
    for (int kc = 0; kc < a.K; kc += kBK) {
        __syncthreads();   // the previous step's fragment reads are done
        As[akq * 4 + 0][am] = ra.x;
        As[akq * 4 + 1][am] = ra.y;
        As[akq * 4 + 2][am] = ra.z;
        As[akq * 4 + 3][am] = ra.w;
        *reinterpret_cast<float4*>(&Bs[bk][bn4 * 4]) = rb;
        __syncthreads();
        if (kc + kBK < a.K) {   // the next step's operands travel while this step's MFMAs run
            ra = load_a(kc + kBK);
            rb = load_b(kc + kBK);
        }
#pragma unroll
        for (int s = 0; s < kBK / 2; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[2 * s + fk][wm + fr], Bs[2 * s + fk][wn + fr], acc, 0, 0, 0);
    }

    // D lane map: col = lane & 31 (cout), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (pixel)
    const int n = n0 + wn + fr;
    if (n < a.Cout) {
        const float bv = a.bias[n];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long long mo = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * fk;
            if (mo < a.M) a.out[(size_t)mo * a.Cout + n] = fmaxf(acc[r] + bv, 0.f);
        }
    }
}

// NHWC [N][H][W][C] -> [N][Ho][Wo][C], Ho = (H - 3) / 2 + 1 (every window is inside the image); one thread per 4 channels
__global__ void lpips_maxpool_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int C4, int Ho, int Wo, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c4 = (int)(i % C4);
    size_t p = i / C4;
    const int ox = (int)(p % Wo);
    p /= Wo;
    const int oy = (int)(p % Ho);
    const size_t n = p / Ho;
    const float4* src = reinterpret_cast<const float4*>(in) + ((n * H + 2 * oy) * W + 2 * ox) * C4 + c4;
    float4 mx = src[0];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const float4 v = src[((size_t)dy * W + dx) * C4];
            mx.x = fmaxf(mx.x, v.x); mx.y = fmaxf(mx.y, v.y); mx.z = fmaxf(mx.z, v.z); mx.w = fmaxf(mx.w, v.w);
        }
    reinterpret_cast<float4*>(out)[i] = mx;
}

__device__ __forceinline__ float wave_sum(float v) {   // fixed butterfly: the same order for every call
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

constexpr int kDistPix = 64;   // pixels per block of lpips_dist_kernel: wave w takes pixels w, w + 4, ... of the block's range
// feat: NHWC [2B][HW][C], image b of in0 at b, of in1 at B + b.  grid = (blocks per image, B); partial[b][blockIdx.x] = sum over the block's pixels
__global__ __launch_bounds__(256) void lpips_dist_kernel(const float* __restrict__ feat, const float* __restrict__ lin, double* __restrict__ partial, int B,
                                                         int HW, int C) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y;
    const float* f0 = feat + (size_t)b * HW * C;
    const float* f1 = feat + (size_t)(B + b) * HW * C;
    const int p_end = min(HW, ((int)blockIdx.x + 1) * kDistPix);
    double acc = 0.0;
    for (int p = blockIdx.x * kDistPix + wave; p < p_end; p += 4) {
        const float* r0 = f0 + (size_t)p * C;
        const float* r1 = f1 + (size_t)p * C;
        float s0 = 0.f, s1 = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float v0 = r0[c], v1 = r1[c];
            s0 = fmaf(v0, v0, s0);
            s1 = fmaf(v1, v1, s1);
        }
        const float d0 = sqrtf(wave_sum(s0)) + 1e-10f, d1 = sqrtf(wave_sum(s1)) + 1e-10f;
        float t = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float d = r0[c] / d0 - r1[c] / d1;
            t = fmaf(lin[c], d * d, t);
        }
        acc += (double)wave_sum(t);
    }
    __shared__ double red[4];
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

inline size_t rup64(size_t n) { return (n + 63) & ~(size_t)63; }

}  // namespace

int lpips_dist_blocks(int hw) { return (hw + kDistPix - 1) / kDistPix; }

LpipsGeom lpips_geometry(int H, int W) {
    if (H < 31 || W < 31) throw HipError("lpips: H and W must be at least 31 (the smallest size at which both 3x3 max-pools have a window)");
    LpipsGeom g;
    int h = H, w = W;
    for (int l = 0; l < 5; ++l) {
        if (l == 1 || l == 2) {   // the max-pool in front of conv2 and conv3
            h = (h - 3) / 2 + 1;
            w = (w - 3) / 2 + 1;
            g.ph[l - 1] = h;
            g.pw[l - 1] = w;
        }
        const LpipsLayer& L = kLpipsLayers[l];
        h = (h + 2 * L.pad - L.k) / L.stride + 1;
        w = (w + 2 * L.pad - L.k) / L.stride + 1;
        g.h[l] = h;
        g.w[l] = w;
    }
    return g;
}

// floats of the tower's workspace for N images: the prepped input, five taps, two pooled maps
size_t lpips_workspace_floats(int N, int H, int W) {
    const LpipsGeom g = lpips_geometry(H, W);
    size_t n = rup64((size_t)N * H * W * 4);
    for (int l = 0; l < 5; ++l) n += rup64((size_t)N * g.h[l] * g.w[l] * kLpipsLayers[l].cout);
    for (int q = 0; q < 2; ++q) n += rup64((size_t)N * g.ph[q] * g.pw[q] * kLpipsLayers[q].cout);
    return n;
}

// The feature tower on N = B (in1 == nullptr) or 2B images; taps[l] point into ws.  mark(desc), if set, is called in front of every launch.
void lpips_features(const LpipsWeights& wt, const float* in0, const float* in1, int B, int H, int W, int normalize, float* ws, float* taps[5],
                    hipStream_t s, const std::function<void(const char*)>& mark) {
    static const char* const conv_names[5] = {"lpips conv1 11x11 s4 3(4)->64 + relu", "lpips conv2 5x5 64->192 + relu", "lpips conv3 3x3 192->384 + relu",
                                              "lpips conv4 3x3 384->256 + relu", "lpips conv5 3x3 256->256 + relu"};
    const LpipsGeom g = lpips_geometry(H, W);
    const int N = in1 ? 2 * B : B;
    if ((long long)N * H * W > (1ll << 31) - 1) throw HipError("lpips: batch x image size beyond 2^31 - 1 pixels");
    float* x0 = ws;
    float* cur = ws + rup64((size_t)N * H * W * 4);
    if (mark) mark("lpips prologue: scale, NCHW -> NHWC4");
    hipLaunchKernelGGL(lpips_prologue_kernel, dim3((unsigned)(((size_t)N * H * W + 255) / 256)), dim3(256), 0, s, in0, in1, x0, B, H * W, N, normalize);
    IRSDE_HIP_CHECK(hipGetLastError());
    const float* src = x0;
    int sh = H, sw = W;
    for (int l = 0; l < 5; ++l) {
        const LpipsLayer& L = kLpipsLayers[l];
        if (l == 1 || l == 2) {
            const int ph = g.ph[l - 1], pw = g.pw[l - 1], C4 = L.cin / 4;   // (64 / 192: no padding)
            const size_t total = (size_t)N * ph * pw * C4;
            if (mark) mark(l == 1 ? "lpips maxpool 3x3 s2 (64)" : "lpips maxpool 3x3 s2 (192)");
            hipLaunchKernelGGL(lpips_maxpool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, cur, sh, sw, C4, ph, pw, total);
            IRSDE_HIP_CHECK(hipGetLastError());
            src = cur;
            cur += rup64(total * 4);
            sh = ph;
            sw = pw;
        }
        LpipsConvArgs a;
        a.in = src; a.w = wt.w[l]; a.bias = wt.bias[l]; a.out = cur;
        a.Hin = sh; a.Win = sw; a.Cin = lpips_cin_padded(l); a.Ho = g.h[l]; a.Wo = g.w[l]; a.Cout = L.cout;
        a.KH = a.KW = L.k; a.stride = L.stride; a.pad = L.pad; a.K = L.k * L.k * a.Cin;
        a.M = (long long)N * g.h[l] * g.w[l];
        if (mark) mark(conv_names[l]);
        hipLaunchKernelGGL(lpips_conv_kernel, dim3((unsigned)((a.M + kBM - 1) / kBM), (unsigned)((L.cout + kBN - 1) / kBN)), dim3(256), 0, s, a);
        IRSDE_HIP_CHECK(hipGetLastError());
        taps[l] = cur;
        src = cur;
        cur += rup64((size_t)a.M * L.cout);
        sh = g.h[l];
        sw = g.w[l];
    }
}

// partial: device doubles, tap l at offset sum_{j < l} B * lpips_dist_blocks(h_j w_j), laid out [B][blocks]
void lpips_distances(const LpipsWeights& wt, float* const taps[5], int B, int H, int W, double* partial, hipStream_t s,
                     const std::function<void(const char*)>& mark) {
    const LpipsGeom g = lpips_geometry(H, W);
    if (B > 65535) throw HipError("lpips: at most 65535 pairs per call");
    if (mark) mark("lpips distance, 5 taps");
    size_t off = 0;
    for (int l = 0; l < 5; ++l) {
        const int hw = g.h[l] * g.w[l], nb = lpips_dist_blocks(hw);
        hipLaunchKernelGGL(lpips_dist_kernel, dim3(nb, B), dim3(256), 0, s, taps[l], wt.lin[l], partial + off, B, hw, kLpipsLayers[l].cout);
        IRSDE_HIP_CHECK(hipGetLastError());
        off += (size_t)B * nb;
    }
}

}  // namespace irsde
