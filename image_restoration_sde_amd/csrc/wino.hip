// Winograd F(m x m, 3x3), m = 2 (default) or 4 (opt-in), for the wide 3x3 stride-1 convolutions of the score network.
//   Y = A^T [ sum_c (G g G^T) .* (B^T d B) ] A         (Lavin & Gray, "Fast Algorithms for Convolutional Neural
//                                                        Networks", CVPR 2016; fp32 throughout)
//   m = 2: 16 products per 4 outputs  (2.25x fewer multiplies than direct), V/M tensors 4x    the input/output size
//   m = 4: 36 products per 16 outputs (4x    fewer multiplies),             V/M tensors 2.25x the input/output size,
//          ~15-30x the rounding error of the direct kernel (1e-5 instead of 5e-7 relative per layer)
// Three launches per convolution:
//   wino_input_kernel   V[k][tile][c]  = (B^T d B)_k   of every (m+2)x(m+2) input patch (stride m); both concat sources
//                                         and the fused nearest-x2 upsample are gathered here          (HBM bound)
//   conv_igemm_kernel   M[k][tile][n]  = sum_c V[k][tile][c] * U[k][n][c], (m+2)^2 independent GEMMs (blockIdx.z = k) on
//                                         the fp32 MFMA pipe — the same kernel as the direct path, run as a 1x1 conv
//   wino_output_kernel  y = A^T M A (m x m pixels per tile) + bias / FiLM / SiLU / residual            (HBM bound)
// U = G g G^T is computed once at weight-load time (engine_weights.hip).
// Polyphase F(4x4,2x2) for the resampling convolutions (4x4 stride 2; nearest x2 + 3x3): wino_poly_input_kernel / wino_poly_output_kernel below, the same
// component GEMMs with 25 / 100 components (WinoPolyParams, common.h).
#include "common.h"

namespace irsde {
namespace {

__device__ __forceinline__ float4 operator+(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 operator-(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float4 operator*(float s, float4 a) { return make_float4(s * a.x, s * a.y, s * a.z, s * a.w); }
__device__ __forceinline__ float silu1(float v) { return v / (1.0f + expf(-v)); }
// V = float4 (4 channels per thread) or float (1 channel per thread: ~90 instead of 170-220 VGPRs, so that transform waves
// can share a SIMD with the resident GEMM waves of another stream; 64 lanes x 4 B is still a 256-byte coalesced access)
template <typename V> struct VecOps;
template <> struct VecOps<float4> {
    static constexpr int N = 4;
    static __device__ __forceinline__ float4 zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
    static __device__ __forceinline__ float4 one() { return make_float4(1.f, 1.f, 1.f, 1.f); }
    static __device__ __forceinline__ float4 mad(float4 v, float4 a, float4 b) { return make_float4(v.x * a.x + b.x, v.y * a.y + b.y, v.z * a.z + b.z, v.w * a.w + b.w); }
    static __device__ __forceinline__ float4 silu(float4 v) { return make_float4(silu1(v.x), silu1(v.y), silu1(v.z), silu1(v.w)); }
};
template <> struct VecOps<float> {
    static constexpr int N = 1;
    static __device__ __forceinline__ float zero() { return 0.f; }
    static __device__ __forceinline__ float one() { return 1.f; }
    static __device__ __forceinline__ float mad(float v, float a, float b) { return v * a + b; }
    static __device__ __forceinline__ float silu(float v) { return silu1(v); }
};

// one application of B^T (input side) / A^T (output side) along one axis
template <int TILE, typename V>
__device__ __forceinline__ void bt_apply(const V* d, V* t) {
    if constexpr (TILE == 2) {  // B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]
        t[0] = d[0] - d[2];
        t[1] = d[1] + d[2];
        t[2] = d[2] - d[1];
        t[3] = d[1] - d[3];
    } else {  // B^T = [4 0 -5 0 1 0; 0 -4 -4 1 1 0; 0 4 -4 -1 1 0; 0 -2 -1 2 1 0; 0 2 -1 -2 1 0; 0 4 0 -5 0 1]
        t[0] = 4.0f * d[0] - 5.0f * d[2] + d[4];
        t[1] = (d[3] + d[4]) - 4.0f * (d[1] + d[2]);
        t[2] = 4.0f * (d[1] - d[2]) + (d[4] - d[3]);
        t[3] = 2.0f * (d[3] - d[1]) + (d[4] - d[2]);
        t[4] = 2.0f * (d[1] - d[3]) + (d[4] - d[2]);
        t[5] = 4.0f * d[1] - 5.0f * d[3] + d[5];
    }
}
template <int TILE, typename V>
__device__ __forceinline__ void at_apply(const V* m, V* y) {
    if constexpr (TILE == 2) {  // A^T = [1 1 1 0; 0 1 -1 -1]
        y[0] = m[0] + m[1] + m[2];
        y[1] = m[1] - m[2] - m[3];
    } else {  // A^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1]
        const V s12 = m[1] + m[2], d12 = m[1] - m[2], s34 = m[3] + m[4], d34 = m[3] - m[4];
        y[0] = m[0] + s12 + s34;
        y[1] = d12 + 2.0f * d34;
        y[2] = s12 + 4.0f * s34;
        y[3] = d12 + 8.0f * d34 + m[5];
    }
}

template <int TILE, typename V>
__global__ __launch_bounds__(256) void wino_input_kernel(const WinoParams p) {
    constexpr int A = TILE + 2;
    constexpr int VN = VecOps<V>::N;
    const int C4 = (p.C0 + p.C1) / VN;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)p.T * C4;
    if (idx >= total) return;
    const int cg = (int)(idx % C4);
    const int t = (int)(idx / C4);
    const int tx = t % p.TW;
    const int t1 = t / p.TW;
    const int ty = t1 % p.TH;
    const int b = t1 / p.TH;
    const int c = cg * VN;
    const float* src;
    int pix;
    if (c < p.C0) {
        src = p.in0 + c; pix = p.C0;
    } else {
        src = p.in1 + (c - p.C0); pix = p.C1;
    }
    const int Hv = p.Hin << p.in_shift, Wv = p.Win << p.in_shift;
    V w[A][A];  // after the row pass: w[r][s] = (B^T d)[r][s]
    {
        V d[A][A];
#pragma unroll
        for (int r = 0; r < A; ++r) {
            const int iy = TILE * ty - 1 + r;
#pragma unroll
            for (int s = 0; s < A; ++s) {
                const int ix = TILE * tx - 1 + s;
                const bool ok = (unsigned)iy < (unsigned)Hv && (unsigned)ix < (unsigned)Wv;
                const size_t pixel = (size_t)b * p.Hin * p.Win + (size_t)((ok ? iy : 0) >> p.in_shift) * p.Win +
                                     ((ok ? ix : 0) >> p.in_shift);
                const V v = *reinterpret_cast<const V*>(src + pixel * pix);
                d[r][s] = ok ? v : VecOps<V>::zero();
            }
        }
#pragma unroll
        for (int s = 0; s < A; ++s) {
            V col[A], tc[A];
#pragma unroll
            for (int r = 0; r < A; ++r) col[r] = d[r][s];
            bt_apply<TILE, V>(col, tc);
#pragma unroll
            for (int r = 0; r < A; ++r) w[r][s] = tc[r];
        }
    }
    const size_t Ctot = (size_t)(p.C0 + p.C1);
    float* vp = p.V + (size_t)t * Ctot + c;
    const size_t kstride = (size_t)p.T * Ctot;
#pragma unroll
    for (int r = 0; r < A; ++r) {
        V o[A];
        bt_apply<TILE, V>(w[r], o);
#pragma unroll
        for (int s = 0; s < A; ++s) *reinterpret_cast<V*>(vp + (size_t)(r * A + s) * kstride) = o[s];
    }
}

// Split-operand mode (gemm_split.hip): the same F(4x4,3x3) input transform, 4 channels per thread, but every V element is
// written as NPL 16-bit pieces (round to nearest even, residual exact in f32): 2 NPL bytes per element instead
// of 4, and the component GEMMs become 16-bit GEMMs with f32-equivalent (NPL = 3, fp16 pairs) or 16-bit (bf16 pairs) operands.
// PAIRS: two pieces pair-interleaved (gemm_split2i_kernel's operands)
// TRI: the three planes in the row-pair-interleaved layout of split3_layout.h (gemm_split3i_kernel's operands)
template <int NPL, bool PAIRS = false, bool F16 = false, bool TRI = false>
__global__ __launch_bounds__(256) void wino_input_split_kernel(const WinoParams p) {
    static_assert(TRI != PAIRS && (!TRI || (NPL == 3 && !F16)) && (!PAIRS || NPL == 2), "three bf16 pieces, or a pair");
    constexpr int A = 6;
    const int C4 = (p.C0 + p.C1) / 4;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)p.T * C4;
    if (idx >= total) return;
    const int cg = (int)(idx % C4);
    const int t = (int)(idx / C4);
    const int tx = t % p.TW;
    const int t1 = t / p.TW;
    const int ty = t1 % p.TH;
    const int b = t1 / p.TH;
    const int c = cg * 4;
    const float* src;
    int pix;
    if (c < p.C0) {
        src = p.in0 + c; pix = p.C0;
    } else {
        src = p.in1 + (c - p.C0); pix = p.C1;
    }
    const int Hv = p.Hin << p.in_shift, Wv = p.Win << p.in_shift;
    float4 w[A][A];
    {
        float4 d[A][A];
#pragma unroll
        for (int r = 0; r < A; ++r) {
            const int iy = 4 * ty - 1 + r;
#pragma unroll
            for (int s = 0; s < A; ++s) {
                const int ix = 4 * tx - 1 + s;
                const bool ok = (unsigned)iy < (unsigned)Hv && (unsigned)ix < (unsigned)Wv;
                const size_t pixel = (size_t)b * p.Hin * p.Win + (size_t)((ok ? iy : 0) >> p.in_shift) * p.Win +
                                     ((ok ? ix : 0) >> p.in_shift);
                const float4 v = *reinterpret_cast<const float4*>(src + pixel * pix);
                d[r][s] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int s = 0; s < A; ++s) {
            float4 col[A], tc[A];
#pragma unroll
            for (int r = 0; r < A; ++r) col[r] = d[r][s];
            bt_apply<4, float4>(col, tc);
#pragma unroll
            for (int r = 0; r < A; ++r) w[r][s] = tc[r];
        }
    }
    const size_t Ctot = (size_t)(p.C0 + p.C1);
    // PAIRS: [component][tile][c / 32][plane][c % 32] (both pieces of a 32-channel block in one 128-byte line)
    unsigned short* vp = TRI ? p.Vs + split3_index((size_t)t, (size_t)c, 0, Ctot / 32) : p.Vs + ((size_t)t * (Ctot / 32) + c / 32) * 64 + (c & 31);
    const size_t kstride = TRI ? split3_comp_elems((size_t)p.T, Ctot) : (size_t)p.T * Ctot * 2;
    constexpr size_t plstride = 32;   // both layouts: the pieces of a 32-channel block sit side by side
#pragma unroll
    for (int r = 0; r < A; ++r) {
        float4 o[A];
        bt_apply<4, float4>(w[r], o);
#pragma unroll
        for (int s = 0; s < A; ++s) {
            float rem[4] = {o[s].x, o[s].y, o[s].z, o[s].w};
            if constexpr (F16) {
#pragma unroll
                for (int e = 0; e < 4; ++e) rem[e] *= p.v_scale;
            }
#pragma unroll
            for (int pl = 0; pl < NPL; ++pl) {
                unsigned short q[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if constexpr (F16) {
                        const _Float16 hb = (_Float16)rem[e];
                        q[e] = __builtin_bit_cast(unsigned short, hb);
                        rem[e] -= (float)hb;
                    } else {
                        const __bf16 hb = (__bf16)rem[e];
                        q[e] = __builtin_bit_cast(unsigned short, hb);
                        rem[e] -= (float)hb;
                    }
                }
                uint2 pk;
                pk.x = (unsigned)q[0] | ((unsigned)q[1] << 16);
                pk.y = (unsigned)q[2] | ((unsigned)q[3] << 16);
                *reinterpret_cast<uint2*>(vp + (size_t)pl * plstride + (size_t)(r * A + s) * kstride) = pk;
            }
        }
    }
}

template <int TILE, typename V>
__global__ __launch_bounds__(256) void wino_output_kernel(const WinoParams p) {
    constexpr int A = TILE + 2;
    constexpr int VN = VecOps<V>::N;
    const int N4 = p.Cout / VN;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)p.T * N4;
    if (idx >= total) return;
    const int ng = (int)(idx % N4);
    const int t = (int)(idx / N4);
    const int tx = t % p.TW;
    const int t1 = t / p.TW;
    const int ty = t1 % p.TH;
    const int b = t1 / p.TH;
    const int n = ng * VN;
    const float* mp = p.M + (size_t)t * p.Cout + n;
    const size_t kstride = (size_t)p.T * p.Cout;
    V u[TILE][A];  // u = A^T m (row pass)
    {
        V m[A][A];
#pragma unroll
        for (int r = 0; r < A; ++r)
#pragma unroll
            for (int s = 0; s < A; ++s) m[r][s] = *reinterpret_cast<const V*>(mp + (size_t)(r * A + s) * kstride);
#pragma unroll
        for (int s = 0; s < A; ++s) {
            V col[A], yc[TILE];
#pragma unroll
            for (int r = 0; r < A; ++r) col[r] = m[r][s];
            at_apply<TILE, V>(col, yc);
#pragma unroll
            for (int i = 0; i < TILE; ++i) u[i][s] = yc[i];
        }
    }
    V bias = VecOps<V>::zero(), sc = VecOps<V>::one(), sh = VecOps<V>::zero();
    if (p.bias) bias = *reinterpret_cast<const V*>(p.bias + n);
    if (p.film) {
        const float* f = p.film + (size_t)(p.film_bstride ? b : 0) * p.film_bstride;
        sc = *reinterpret_cast<const V*>(f + n) + VecOps<V>::one();
        sh = *reinterpret_cast<const V*>(f + p.Cout + n);
    }
    const int Ho = TILE * p.TH, Wo = TILE * p.TW;
#pragma unroll
    for (int i = 0; i < TILE; ++i) {
        V y[TILE];
        at_apply<TILE, V>(u[i], y);
#pragma unroll
        for (int j = 0; j < TILE; ++j) {
            const size_t pixel = ((size_t)b * Ho + TILE * ty + i) * Wo + TILE * tx + j;
            V v = y[j] + bias;
            if (p.film) v = VecOps<V>::mad(v, sc, sh);
            if (p.silu) v = VecOps<V>::silu(v);
            if (p.res) v = v + *reinterpret_cast<const V*>(p.res + pixel * p.res_stride + n);
            *reinterpret_cast<V*>(p.out + pixel * p.out_stride + n) = v;
        }
    }
}

// ---- polyphase F(4x4,2x2) (points 0, 1, -1, 2, inf): the stride-2 4x4 and the nearest-x2 + 3x3 convolutions, see WinoPolyParams ----
// B^T = [2 -1 -2 1 0; 0 -2 -1 1 0; 0 2 -3 1 0; 0 -1 0 1 0; 0 2 -1 -2 1]
__device__ __forceinline__ void bt5_apply(const float4* d, float4* t) {
    t[0] = 2.0f * (d[0] - d[2]) + (d[3] - d[1]);
    t[1] = (d[3] - d[2]) - 2.0f * d[1];
    t[2] = 2.0f * d[1] - 3.0f * d[2] + d[3];
    t[3] = d[3] - d[1];
    t[4] = 2.0f * (d[1] - d[3]) + (d[4] - d[2]);
}
// A^T = [1 1 1 1 0; 0 1 -1 2 0; 0 1 1 4 0; 0 1 -1 8 1]
__device__ __forceinline__ void at5_apply(const float4* m, float4* y) {
    const float4 s12 = m[1] + m[2], d12 = m[1] - m[2];
    y[0] = m[0] + s12 + m[3];
    y[1] = d12 + 2.0f * m[3];
    y[2] = s12 + 4.0f * m[3];
    y[3] = d12 + 8.0f * m[3] + m[4];
}

// one thread = (tile, phase, 4 channels): the phase's 5x5 patch (down: every second pixel from (8 ty - 1 + p, 8 tx - 1 + q); up: from (4 ty - 1 + py, 4 tx - 1 + px))
// TRI: V as three bf16 pieces in the layout of split3_layout.h (p.Vs) instead of f32 (p.V)
// LINES (UP and TRI): the whole-line writer.  Sixteen threads form a group = (tile pair, phase, 32-k block): 2 tiles x 8 channel quads, i.e. what one
// 384-byte row-pair block of every component holds, and a work-group is 16 groups (consecutive 32-k blocks first).  Same loads, same bt5_apply order and the
// same round-to-nearest-even splitting per thread, but the pieces of five components at a time (one r) go through LDS, and the work-group then stores them
// 16 bytes per lane at consecutive addresses: whole 384-byte blocks, neighbouring 32-k blocks of a component back to back, instead of 8 bytes per thread and
// plane into 64-byte runs with the two rows of a block coming from different waves.  The pad row of an odd T stays unwritten.
constexpr int kPolyLinesGroups = 16;
template <bool UP, bool TRI = false, bool LINES = false>
__global__ __launch_bounds__(256) void wino_poly_input_kernel(const WinoPolyParams p) {
    static_assert(!LINES || (UP && TRI), "the whole-line writer exists for the Upsample triples");
    __shared__ uint4 stage[LINES ? kPolyLinesGroups * 5 * 24 : 1];
    const int C4 = p.C / 4;
    int c, ph, t;
    bool active = true;
    if constexpr (LINES) {
        const int nkb = p.C / 32, sub = threadIdx.x & 15;
        const long long grp = (long long)blockIdx.x * kPolyLinesGroups + (threadIdx.x >> 4);
        const long long u = grp / (4 * nkb);
        c = (int)(grp % nkb) * 32 + (sub & 7) * 4;
        ph = (int)((grp / nkb) & 3);
        const long long tt = 2 * u + (sub >> 3);
        active = tt < p.T;
        t = (int)(active ? tt : p.T - 1);   // (an idle thread loads a valid tile and stores nothing: it still has to reach the barriers)
    } else {
        const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
        const long long total = (long long)p.T * 4 * C4;
        if (idx >= total) return;
        c = (int)(idx % C4) * 4;
        const long long i1 = idx / C4;
        ph = (int)(i1 & 3);
        t = (int)(i1 >> 2);
    }
    const int tx = t % p.TW;
    const int t1 = t / p.TW;
    const int ty = t1 % p.TH;
    const int b = t1 / p.TH;
    constexpr int STEP = UP ? 1 : 2;
    const int y0 = 4 * STEP * ty - 1 + (ph >> 1), x0 = 4 * STEP * tx - 1 + (ph & 1);
    const float* src = p.in + c;
    float4 w[5][5];  // after the row pass: w[r][s] = (B^T d)[r][s]
    {
        float4 d[5][5];
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            const int iy = y0 + STEP * r;
#pragma unroll
            for (int s = 0; s < 5; ++s) {
                const int ix = x0 + STEP * s;
                const bool ok = (unsigned)iy < (unsigned)p.Hin && (unsigned)ix < (unsigned)p.Win;
                const size_t pixel = (size_t)b * p.Hin * p.Win + (size_t)(ok ? iy : 0) * p.Win + (ok ? ix : 0);
                const float4 v = *reinterpret_cast<const float4*>(src + pixel * p.C);
                d[r][s] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int s = 0; s < 5; ++s) {
            float4 col[5], tc[5];
#pragma unroll
            for (int r = 0; r < 5; ++r) col[r] = d[r][s];
            bt5_apply(col, tc);
#pragma unroll
            for (int r = 0; r < 5; ++r) w[r][s] = tc[r];
        }
    }
    const size_t K = UP ? (size_t)p.C : (size_t)4 * p.C;
    const size_t kstride = (size_t)p.T * K;
    float* vp = UP ? p.V + (size_t)ph * 25 * kstride + (size_t)t * K + c : p.V + (size_t)t * K + (size_t)ph * p.C + c;
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        float4 o[5];
        bt5_apply(w[r], o);
#pragma unroll
        for (int s = 0; s < 5; ++s) {
            if constexpr (TRI) {
                const size_t z = (UP ? (size_t)ph * 25 : 0) + (size_t)(r * 5 + s);
                // LINES: the group's 384-byte block of component s of this r in LDS, laid out as in memory: [tile parity][plane][32 k]
                unsigned short* q = LINES ? reinterpret_cast<unsigned short*>(stage) + ((threadIdx.x >> 4) * 5 + s) * 192 + ((threadIdx.x >> 3) & 1) * 96 + (threadIdx.x & 7) * 4
                                          : p.Vs + z * split3_comp_elems((size_t)p.T, K) + split3_index((size_t)t, UP ? (size_t)c : (size_t)ph * p.C + c, 0, K / 32);
                float rem[4] = {o[s].x, o[s].y, o[s].z, o[s].w};
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) {
                    unsigned short b[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const __bf16 hb = (__bf16)rem[e];
                        b[e] = __builtin_bit_cast(unsigned short, hb);
                        rem[e] -= (float)hb;
                    }
                    uint2 pk;
                    pk.x = (unsigned)b[0] | ((unsigned)b[1] << 16);
                    pk.y = (unsigned)b[2] | ((unsigned)b[3] << 16);
                    *reinterpret_cast<uint2*>(q + pl * 32) = pk;
                }
            } else {
                *reinterpret_cast<float4*>(vp + (size_t)(r * 5 + s) * kstride) = o[s];
            }
        }
        if constexpr (LINES) {
            __syncthreads();
            const int nkb = p.C / 32;
            const long long ngroups = (long long)((p.T + 1) / 2) * 4 * nkb;
            // 16-byte chunk i of this r: component s = i / 384, group (i % 384) / 24, chunk i % 24 of its block (12 per tile row)
            for (int i = threadIdx.x; i < 5 * kPolyLinesGroups * 24; i += 256) {
                const int s = i / (kPolyLinesGroups * 24), gl = (i / 24) % kPolyLinesGroups, ch = i % 24;
                const long long grp = (long long)blockIdx.x * kPolyLinesGroups + gl;
                if (grp >= ngroups) continue;
                const long long u = grp / (4 * nkb);
                if (ch >= 12 && 2 * u + 1 >= p.T) continue;   // the pad row of an odd T
                const size_t z = (size_t)((grp / nkb) & 3) * 25 + (size_t)(r * 5 + s);
                unsigned short* dst = p.Vs + z * split3_comp_elems((size_t)p.T, K) + ((size_t)u * nkb + (size_t)(grp % nkb)) * 192 + ch * 8;
                *reinterpret_cast<uint4*>(dst) = stage[(gl * 5 + s) * 24 + ch];
            }
            __syncthreads();
        }
    }
}

// one thread = (tile, [up: output phase,] 4 output channels): y = A^T m A + bias, 4x4 pixels (up: of the phase's pixel lattice)
template <bool UP>
__global__ __launch_bounds__(256) void wino_poly_output_kernel(const WinoPolyParams p) {
    const int N4 = p.Cout / 4;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)p.T * (UP ? 4 : 1) * N4;
    if (idx >= total) return;
    const int n = (int)(idx % N4) * 4;
    const long long i1 = idx / N4;
    const int ph = UP ? (int)(i1 & 3) : 0;
    const int t = UP ? (int)(i1 >> 2) : (int)i1;
    const int tx = t % p.TW;
    const int t1 = t / p.TW;
    const int ty = t1 % p.TH;
    const int b = t1 / p.TH;
    const size_t kstride = (size_t)p.T * p.Cout;
    const float* mp = p.M + (size_t)ph * 25 * kstride + (size_t)t * p.Cout + n;
    float4 u[4][5];  // u = A^T m (row pass)
    {
        float4 m[5][5];
#pragma unroll
        for (int r = 0; r < 5; ++r)
#pragma unroll
            for (int s = 0; s < 5; ++s) m[r][s] = *reinterpret_cast<const float4*>(mp + (size_t)(r * 5 + s) * kstride);
#pragma unroll
        for (int s = 0; s < 5; ++s) {
            float4 col[5], yc[4];
#pragma unroll
            for (int r = 0; r < 5; ++r) col[r] = m[r][s];
            at5_apply(col, yc);
#pragma unroll
            for (int i = 0; i < 4; ++i) u[i][s] = yc[i];
        }
    }
    float4 bias = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.bias) bias = *reinterpret_cast<const float4*>(p.bias + n);
    const int LH = UP ? p.Hin : p.Ho, LW = UP ? p.Win : p.Wo;   // extent of the tiled lattice
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float4 y[4];
        at5_apply(u[i], y);
        const int ly = 4 * ty + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int lx = 4 * tx + j;
            if (ly >= LH || lx >= LW) continue;
            const int oy = UP ? 2 * ly + (ph >> 1) : ly, ox = UP ? 2 * lx + (ph & 1) : lx;
            const size_t pixel = ((size_t)b * p.Ho + oy) * p.Wo + ox;
            *reinterpret_cast<float4*>(p.out + pixel * p.out_stride + n) = y[j] + bias;
        }
    }
}

}  // namespace

static void wino_poly_check(const WinoPolyParams& p, bool output) {
    const int LH = p.up ? p.Hin : p.Ho, LW = p.up ? p.Win : p.Wo;
    if (p.C <= 0 || p.C % 4 || p.B <= 0 || p.Hin <= 0 || p.Win <= 0 || p.TH != (LH + 3) / 4 || p.TW != (LW + 3) / 4 || p.T != p.B * p.TH * p.TW)
        throw HipError("wino_poly: inconsistent tiling");
    if (p.up ? (p.Ho != 2 * p.Hin || p.Wo != 2 * p.Win) : (p.Ho != (p.Hin - 2) / 2 + 1 || p.Wo != (p.Win - 2) / 2 + 1 || p.Hin < 2 || p.Win < 2))
        throw HipError("wino_poly: output size does not belong to the input size");
    if (output && (p.Cout <= 0 || p.Cout % 4 || p.out_stride % 4 || p.out_stride < p.Cout)) throw HipError("wino_poly_output: channels must be multiples of 4");
}

void launch_wino_poly_input(const WinoPolyParams& p, hipStream_t s) {
    wino_poly_check(p, false);
    const long long total = (long long)p.T * p.C;   // T * 4 phases * C / 4
    const dim3 grid((unsigned)((total + 255) / 256));
    if (p.Vs) {
        if (p.C % 32) throw HipError("wino_poly_input (triples): channels must be a multiple of 32");
        static const int lines = tuning_env_int("IRSDE_WINO_POLY_LINES", 1);
        if (p.up && lines && !p.thread_writer) {   // the whole-line writer: 16 groups of (tile pair, phase, 32-k block) per work-group
            const long long groups = (long long)((p.T + 1) / 2) * 4 * (p.C / 32);
            hipLaunchKernelGGL((wino_poly_input_kernel<true, true, true>), dim3((unsigned)((groups + kPolyLinesGroups - 1) / kPolyLinesGroups)), dim3(256), 0, s, p);
        } else if (p.up) hipLaunchKernelGGL((wino_poly_input_kernel<true, true>), grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL((wino_poly_input_kernel<false, true>), grid, dim3(256), 0, s, p);
    } else if (p.up) hipLaunchKernelGGL((wino_poly_input_kernel<true>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((wino_poly_input_kernel<false>), grid, dim3(256), 0, s, p);
    IRSDE_HIP_CHECK(hipGetLastError());
}

void launch_wino_poly_output(const WinoPolyParams& p, hipStream_t s) {
    wino_poly_check(p, true);
    const long long total = (long long)p.T * (p.up ? 4 : 1) * (p.Cout / 4);
    const dim3 grid((unsigned)((total + 255) / 256));
    if (p.up) hipLaunchKernelGGL((wino_poly_output_kernel<true>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((wino_poly_output_kernel<false>), grid, dim3(256), 0, s, p);
    IRSDE_HIP_CHECK(hipGetLastError());
}

// U = G g G^T of F(4x4,2x2), G = [1/2 0; -1/2 -1/2; -1/6 1/6; 1/6 1/3; 0 1], per phase, in double, rounded once (host, at weight load)
void wino_poly_transform_weights(const float* w_packed, int Cout, int Cin, float* U, int up) {
    static const double G[5][2] = {{0.5, 0.0}, {-0.5, -0.5}, {-1.0 / 6, 1.0 / 6}, {1.0 / 6, 1.0 / 3}, {0.0, 1.0}};
    const int KW = up ? 3 : 4;
    const size_t K = up ? (size_t)Cin : (size_t)4 * Cin;
    const size_t kstride = (size_t)Cout * K;
    for (int n = 0; n < Cout; ++n)
        for (int c = 0; c < Cin; ++c) {
            double w[4][4];
            for (int ky = 0; ky < KW; ++ky)
                for (int kx = 0; kx < KW; ++kx) w[ky][kx] = w_packed[(((size_t)n * KW + ky) * KW + kx) * Cin + c];
            for (int ph = 0; ph < 4; ++ph) {
                const int p = ph >> 1, q = ph & 1;
                double g[2][2];
                for (int a = 0; a < 2; ++a)
                    for (int b = 0; b < 2; ++b) {
                        if (!up) {
                            g[a][b] = w[2 * a + p][2 * b + q];
                        } else {   // rows: phase 0 taps {w0, w1 + w2} on rows {i - 1, i}; phase 1 taps {w0 + w1, w2} on rows {i, i + 1}; columns alike
                            const int y0 = p == 0 ? (a == 0 ? 0 : 1) : (a == 0 ? 0 : 2), y1 = p == 0 ? (a == 0 ? 0 : 2) : (a == 0 ? 1 : 2);
                            const int x0 = q == 0 ? (b == 0 ? 0 : 1) : (b == 0 ? 0 : 2), x1 = q == 0 ? (b == 0 ? 0 : 2) : (b == 0 ? 1 : 2);
                            double sum = 0.0;
                            for (int ky = y0; ky <= y1; ++ky)
                                for (int kx = x0; kx <= x1; ++kx) sum += w[ky][kx];
                            g[a][b] = sum;
                        }
                    }
                double tmp[5][2];
                for (int r = 0; r < 5; ++r)
                    for (int b = 0; b < 2; ++b) tmp[r][b] = G[r][0] * g[0][b] + G[r][1] * g[1][b];
                for (int r = 0; r < 5; ++r)
                    for (int s = 0; s < 5; ++s) {
                        const float v = (float)(tmp[r][0] * G[s][0] + tmp[r][1] * G[s][1]);
                        if (up) U[((size_t)ph * 25 + r * 5 + s) * kstride + (size_t)n * K + c] = v;
                        else U[(size_t)(r * 5 + s) * kstride + (size_t)n * K + (size_t)ph * Cin + c] = v;
                    }
            }
        }
}

// IRSDE_WINO_VEC=1 (experiment): one channel per thread instead of four
static int wino_vec() {
    static const int v = tuning_env_int("IRSDE_WINO_VEC", 4);
    return v;
}

void launch_wino_input(const WinoParams& p, hipStream_t s) {
    if (p.Vs) {  // split-operand mode: 16-bit pieces
        if (p.tile != 4 || (p.C0 % 4) || (p.C1 % 4)) throw HipError("wino_input (split): F(4x4,3x3) only");
        const long long tot = (long long)p.T * ((p.C0 + p.C1) / 4);
        const dim3 gr((unsigned)((tot + 255) / 256));
        if (p.v_triples) {
            if (p.nplanes != 3 || p.v_pairs || p.v_f16 || (p.C0 + p.C1) % 32) throw HipError("wino_input (triples): three bf16 planes, channels a multiple of 32");
            hipLaunchKernelGGL((wino_input_split_kernel<3, false, false, true>), gr, dim3(256), 0, s, p);
        } else {
            if (!p.v_pairs || p.nplanes != 2 || (p.C0 + p.C1) % 32) throw HipError("wino_input (pairs): two planes, channels a multiple of 32");
            if (p.v_f16) hipLaunchKernelGGL((wino_input_split_kernel<2, true, true>), gr, dim3(256), 0, s, p);
            else hipLaunchKernelGGL((wino_input_split_kernel<2, true, false>), gr, dim3(256), 0, s, p);
        }
        IRSDE_HIP_CHECK(hipGetLastError());
        return;
    }
    const int vn = wino_vec() == 1 ? 1 : 4;
    const long long total = (long long)p.T * ((p.C0 + p.C1) / vn);
    const dim3 grid((unsigned)((total + 255) / 256));
    if (p.tile == 4) {
        if (vn == 1) hipLaunchKernelGGL((wino_input_kernel<4, float>), grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL((wino_input_kernel<4, float4>), grid, dim3(256), 0, s, p);
    } else {
        if (vn == 1) hipLaunchKernelGGL((wino_input_kernel<2, float>), grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL((wino_input_kernel<2, float4>), grid, dim3(256), 0, s, p);
    }
    IRSDE_HIP_CHECK(hipGetLastError());
}

void launch_wino_output(const WinoParams& p, hipStream_t s) {
    const int vn = wino_vec() == 1 ? 1 : 4;
    const long long total = (long long)p.T * (p.Cout / vn);
    const dim3 grid((unsigned)((total + 255) / 256));
    if (p.tile == 4) {
        if (vn == 1) hipLaunchKernelGGL((wino_output_kernel<4, float>), grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL((wino_output_kernel<4, float4>), grid, dim3(256), 0, s, p);
    } else {
        if (vn == 1) hipLaunchKernelGGL((wino_output_kernel<2, float>), grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL((wino_output_kernel<2, float4>), grid, dim3(256), 0, s, p);
    }
    IRSDE_HIP_CHECK(hipGetLastError());
}

// U[k][n][c] = (G g G^T)_k;  g given as [Cout][3][3][Cin] (packed layout); tile = 2 or 4 (host, at weight load)
void wino_transform_weights(const float* w_packed, int Cout, int Cin, float* U, int tile) {
    static const float G2[4][3] = {{1.f, 0.f, 0.f}, {0.5f, 0.5f, 0.5f}, {0.5f, -0.5f, 0.5f}, {0.f, 0.f, 1.f}};
    static const float G4[6][3] = {{1.f / 4, 0.f, 0.f},          {-1.f / 6, -1.f / 6, -1.f / 6}, {-1.f / 6, 1.f / 6, -1.f / 6},
                                   {1.f / 24, 1.f / 12, 1.f / 6}, {1.f / 24, -1.f / 12, 1.f / 6}, {0.f, 0.f, 1.f}};
    const int A = tile + 2;
    const float(*G)[3] = tile == 4 ? G4 : G2;
    const size_t kstride = (size_t)Cout * Cin;
    for (int n = 0; n < Cout; ++n)
        for (int c = 0; c < Cin; ++c) {
            double g[3][3];
            for (int ky = 0; ky < 3; ++ky)
                for (int kx = 0; kx < 3; ++kx) g[ky][kx] = w_packed[(((size_t)n * 3 + ky) * 3 + kx) * Cin + c];
            double tmp[6][3];
            for (int r = 0; r < A; ++r)
                for (int kx = 0; kx < 3; ++kx)
                    tmp[r][kx] = (double)G[r][0] * g[0][kx] + (double)G[r][1] * g[1][kx] + (double)G[r][2] * g[2][kx];
            for (int r = 0; r < A; ++r)
                for (int s = 0; s < A; ++s)
                    U[(size_t)(r * A + s) * kstride + (size_t)n * Cin + c] =
                        (float)(tmp[r][0] * G[s][0] + tmp[r][1] * G[s][1] + tmp[r][2] * G[s][2]);
        }
}

}  // namespace irsde
