// TLSC (test-time local statistics conversion) pooling of CNAFNetLocal
// (codes/config/latent-dehazing/models/modules/local_arch.py:25-72, DenoisingNAFNet_arch.py:190-200): the NAFBlock's
// AdaptiveAvgPool2d(1) replaced by the mean over a k1 x k2 window, replicate-padded back to the map.
//
// On the gated tensor g [B][h][w][c] (NHWC fp32) a block with a local window runs
//   1. tlsc_axis_sum_kernel   row pass     r[b][y][j]  = sum_{x = j .. j + k2 - 1} g[b][y][x]          [B][h][nw][c],  nw = w - k2 + 1
//   2. tlsc_axis_sum_kernel   column pass  m[b][i][j]  = sum_{y = i .. i + k1 - 1} r[b][y][j] / (k1 k2)  [B][nh][nw][c], nh = h - k1 + 1
//   3. sca.1 on the compact map m (the engine's 1x1 implicit-GEMM kernel, M = B nh nw rows) -> s [B][nh][nw][c]
//   4. tlsc_scale_kernel      g[b][y][x] *= s[b][clamp(y - top, 0, nh - 1)][clamp(x - left, 0, nw - 1)],  top = (k1 - 1) / 2, left = (k2 - 1) / 2
// Only the nh x nw distinct window means exist, so sca.1 runs on those and the replicate pad is a clamped gather.
//
// Arithmetic: the reference takes differences of a whole-image fp32 prefix sum (cumsum over both axes), whose error grows with h w.
// Here every window sum is separable and local: a lane owns kTlscSeg consecutive outputs along the sliding axis, forms the first
// one as a direct sum of k values and the next kTlscSeg - 1 by adding the entering and subtracting the leaving value, so a running
// sum never lives longer than kTlscSeg - 1 updates.  No atomics, one fixed summation order per output: deterministic, independent
// of B and of how the kernel is launched (eager or from a captured graph).
// Layout: channels innermost, one float4 (16 bytes) per lane and access, consecutive lanes on consecutive channel quads.
#include "common.h"

namespace irsde {

namespace {

constexpr int kTlscSeg = 8;   // outputs per lane along the sliding axis = the restart interval of the running sum

__device__ __forceinline__ float4 f4add(const float4 a, const float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 f4sub(const float4 a, const float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }

// in [outer][len][inner4] float4 -> out [outer][len - k + 1][inner4]: sliding sums of k along `len`, times scale
__global__ __launch_bounds__(256) void tlsc_axis_sum_kernel(const float4* __restrict__ in, float4* __restrict__ out, const long long total,
                                                            const int len, const int k, const int inner4, const int nseg, const float scale) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;   // total = outer * nseg * inner4
    const int q = (int)(idx % inner4);
    const long long t = idx / inner4;
    const int sg = (int)(t % nseg);
    const long long o = t / nseg;
    const int nout = len - k + 1;
    const int j0 = sg * kTlscSeg;                                   // < nout: nseg = ceil(nout / kTlscSeg)
    const int j1 = j0 + kTlscSeg < nout ? j0 + kTlscSeg : nout;
    const float4* ip = in + o * len * inner4 + q;
    float4* op = out + o * nout * inner4 + q;
    float4 acc = ip[(long long)j0 * inner4];
    for (int x = 1; x < k; ++x) acc = f4add(acc, ip[(long long)(j0 + x) * inner4]);       // rows j0 .. j0 + k - 1 <= len - 1
    op[(long long)j0 * inner4] = make_float4(acc.x * scale, acc.y * scale, acc.z * scale, acc.w * scale);
    for (int j = j0 + 1; j < j1; ++j) {                                                   // j + k - 1 <= nout + k - 2 = len - 1
        acc = f4sub(f4add(acc, ip[(long long)(j + k - 1) * inner4]), ip[(long long)(j - 1) * inner4]);
        op[(long long)j * inner4] = make_float4(acc.x * scale, acc.y * scale, acc.z * scale, acc.w * scale);
    }
}

// g [B][h][w][c4] *= s [B][nh][nw][c4] gathered with the replicate pad's clamp
__global__ __launch_bounds__(256) void tlsc_scale_kernel(float4* __restrict__ g, const float4* __restrict__ s, const long long total, const int h,
                                                         const int w, const int c4, const int nh, const int nw, const int top, const int left) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;   // total = B * h * w * c4
    const int q = (int)(idx % c4);
    long long t = idx / c4;
    const int x = (int)(t % w);
    t /= w;
    const int y = (int)(t % h);
    const long long b = t / h;
    int i = y - top, j = x - left;
    i = i < 0 ? 0 : (i > nh - 1 ? nh - 1 : i);
    j = j < 0 ? 0 : (j > nw - 1 ? nw - 1 : j);
    const float4 sc = s[((b * nh + i) * nw + j) * c4 + q];
    float4 v = g[idx];
    v.x *= sc.x; v.y *= sc.y; v.z *= sc.z; v.w *= sc.w;
    g[idx] = v;
}

void axis_sum(const float* in, float* out, long long outer, int len, int k, long long inner, float scale, hipStream_t s) {
    const int nout = len - k + 1, nseg = (nout + kTlscSeg - 1) / kTlscSeg;
    const long long inner4 = inner / 4, total = outer * nseg * inner4;
    if (inner4 >= (1ll << 31) || (total + 255) / 256 >= (1ll << 31)) throw HipError("tlsc: map too large");
    hipLaunchKernelGGL(tlsc_axis_sum_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const float4*>(in),
                       reinterpret_cast<float4*>(out), total, len, k, (int)inner4, nseg, scale);
    IRSDE_HIP_CHECK(hipGetLastError());
}

}  // namespace

void tlsc_check_shape(int B, int h, int w, int c, int k1, int k2) {
    if (B < 1 || h < 1 || w < 1 || c < 4 || c % 4) throw HipError("tlsc: the channel count must be a positive multiple of 4");
    if (k1 < 1 || k2 < 1 || k1 > h || k2 > w) throw HipError("tlsc: the window must lie inside the map");
}

// gated [B][h][w][c] -> rowsum (scratch) [B][h][w - k2 + 1][c] -> pooled [B][h - k1 + 1][w - k2 + 1][c] (window means)
void launch_tlsc_pool(const float* gated, float* rowsum, float* pooled, int B, int h, int w, int c, int k1, int k2, hipStream_t s) {
    tlsc_check_shape(B, h, w, c, k1, k2);
    const int nw = w - k2 + 1;
    axis_sum(gated, rowsum, (long long)B * h, w, k2, c, 1.0f, s);
    axis_sum(rowsum, pooled, B, h, k1, (long long)nw * c, 1.0f / ((float)k1 * (float)k2), s);
}

// gated [B][h][w][c] *= scale [B][h - k1 + 1][w - k2 + 1][c] replicate-padded to h x w (pad top (k1 - 1) / 2, left (k2 - 1) / 2)
void launch_tlsc_scale(float* gated, const float* scale, int B, int h, int w, int c, int k1, int k2, hipStream_t s) {
    tlsc_check_shape(B, h, w, c, k1, k2);
    const long long total = (long long)B * h * w * (c / 4);
    if ((total + 255) / 256 >= (1ll << 31)) throw HipError("tlsc: map too large");
    hipLaunchKernelGGL(tlsc_scale_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, reinterpret_cast<float4*>(gated),
                       reinterpret_cast<const float4*>(scale), total, h, w, c / 4, h - k1 + 1, w - k2 + 1, (k1 - 1) / 2, (k2 - 1) / 2);
    IRSDE_HIP_CHECK(hipGetLastError());
}

}  // namespace irsde
