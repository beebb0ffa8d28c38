// Memory-bound kernels of the IR-SDE score network and sampler for gfx950 (wave64).
//   channel LayerNorm            module_util.py:70-79
//   full softmax attention       module_util.py:182-204   (denoising-sde bottleneck; LinearAttention lives in linear_attn.hip)
//   input prep                   DenoisingUNet_arch.py:90-94 (xt-cond, cat, reflect pad)
//   time embedding / FiLM rows   module_util.py:29-41, DenoisingUNet_arch.py:42-47, module_util.py:127-141
//   reverse-step update + RNG    sde_utils.py:44-48,175-223
//   NAFBlock glue                depthwise conv + SimpleGate, SCA, norm + FiLM + 1x1 convolution; dtype / layout conversions
#include "misc_shared.h"
#include <algorithm>
#include <type_traits>

namespace irsde {

namespace {

// ---------------------------------------------------------------------------------------------
// Channel LayerNorm: y = (x - mean) * (var + eps)^-1/2 * g (+ res), per pixel over C (NHWC: C contiguous).
// L lanes cooperate on one pixel (L = largest power of two <= min(64, C/4)); 64/L pixels per wave.
// Two-pass (mean, then centred variance) in registers, like torch.var/torch.mean.
// ---------------------------------------------------------------------------------------------
constexpr int kLnMaxVec = 8;  // float4 vectors per lane -> C <= 2048

// KV = float4 vectors per lane (1, 2, 4, 8), U = independent pixel groups per iteration: all U x KV loads are issued before the
// first reduction and the U cross-lane reductions interleave — with one pixel group per iteration a wave had a single load
// in flight and the kernel sat at ~2.5 TB/s, latency-bound.
template <typename T, int KV, int U>
__global__ __launch_bounds__(256) void layernorm_kernel(const T* __restrict__ x, const float* __restrict__ g,
                                                        const T* __restrict__ res, T* __restrict__ out,
                                                        const long long M, const int C, const int L, const float eps,
                                                        const float* __restrict__ fscale = nullptr,
                                                        const float* __restrict__ fshift = nullptr,
                                                        const int film_bstride = 0, const long long ppi = 1) {
    const int lane = threadIdx.x & 63;
    const int ppw = 64 / L;
    const int li = lane % L;
    const int sub = lane / L;
    const int nvec = C >> 2;
    const long long wave_id = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    const float invC = 1.0f / (float)C;
    for (long long base = wave_id * ppw * U; base < M; base += nwaves * ppw * U) {
        float4 v[U][KV];
        float s[U], q[U];
        long long pix[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            pix[u] = base + (long long)u * ppw + sub;
            const T* xp = x + (pix[u] < M ? pix[u] : 0) * C;
            s[u] = 0.f;
#pragma unroll
            for (int k = 0; k < KV; ++k) {
                const int vi = li + k * L;
                const float4 t = ld4(xp + 4 * (vi < nvec ? vi : 0));  // unconditional load from a clamped index, then select
                v[u][k] = vi < nvec ? t : make_float4(0.f, 0.f, 0.f, 0.f);
                s[u] += (v[u][k].x + v[u][k].y) + (v[u][k].z + v[u][k].w);
            }
        }
        for (int o = L >> 1; o > 0; o >>= 1)
#pragma unroll
            for (int u = 0; u < U; ++u) s[u] += __shfl_xor(s[u], o, 64);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float mean = s[u] * invC;
            q[u] = 0.f;
#pragma unroll
            for (int k = 0; k < KV; ++k) {
                const int vi = li + k * L;
                if (vi < nvec) {
                    v[u][k].x -= mean; v[u][k].y -= mean; v[u][k].z -= mean; v[u][k].w -= mean;
                    q[u] += (v[u][k].x * v[u][k].x + v[u][k].y * v[u][k].y) + (v[u][k].z * v[u][k].z + v[u][k].w * v[u][k].w);
                }
            }
        }
        for (int o = L >> 1; o > 0; o >>= 1)
#pragma unroll
            for (int u = 0; u < U; ++u) q[u] += __shfl_xor(q[u], o, 64);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (pix[u] >= M) continue;
            const float rstd = 1.0f / sqrtf(q[u] * invC + eps);
            T* op = out + pix[u] * C;
            const float4* gp = reinterpret_cast<const float4*>(g);
            const T* rp = res ? res + pix[u] * C : nullptr;
            const size_t frow = fscale ? (size_t)(film_bstride ? pix[u] / ppi : 0) * film_bstride : 0;
#pragma unroll
            for (int k = 0; k < KV; ++k) {
                const int vi = li + k * L;
                if (vi < nvec) {
                    const float4 gg = gp[vi];
                    float4 o;
                    o.x = v[u][k].x * rstd * gg.x;
                    o.y = v[u][k].y * rstd * gg.y;
                    o.z = v[u][k].z * rstd * gg.z;
                    o.w = v[u][k].w * rstd * gg.w;
                    if (fscale) {  // NAFNet: x * (scale + 1) + shift  (DenoisingNAFNet_arch.py:64,75)
                        const float4 s4 = reinterpret_cast<const float4*>(fscale + frow)[vi];
                        const float4 h4 = reinterpret_cast<const float4*>(fshift + frow)[vi];
                        o.x = o.x * (s4.x + 1.0f) + h4.x; o.y = o.y * (s4.y + 1.0f) + h4.y;
                        o.z = o.z * (s4.z + 1.0f) + h4.z; o.w = o.w * (s4.w + 1.0f) + h4.w;
                    }
                    if (rp) {
                        const float4 r = ld4(rp + 4 * vi);
                        o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w;
                    }
                    st4(op + 4 * vi, o);
                }
            }
        }
    }
}

template <typename T>
static void launch_ln_t(const T* x, const float* g, const T* res, T* out, int64_t M, int C, float eps, const float* fscale,
                        const float* fshift, int film_bstride, int64_t ppi, hipStream_t s) {
    if (C % 4 || C > 4 * 64 * kLnMaxVec) throw HipError("layernorm: unsupported channel count " + std::to_string(C));
    int L = 1;
    while (L * 2 <= 64 && L * 2 <= C / 4) L *= 2;
    const int need = (C / 4 + L - 1) / L;
    if (need > kLnMaxVec) throw HipError("layernorm: channel count too large");
    const int ppw = 64 / L;
    const int U = need <= 2 ? 4 : (need <= 4 ? 2 : 1);
    const int64_t waves = (M + (int64_t)ppw * U - 1) / ((int64_t)ppw * U);
    int64_t blocks = (waves + 3) / 4;
    if (blocks > 256 * 8) blocks = 256 * 8;
    if (blocks < 1) blocks = 1;
    const dim3 grid((unsigned)blocks), blk(256);
#define IRSDE_LN(KV, UU) hipLaunchKernelGGL((layernorm_kernel<T, KV, UU>), grid, blk, 0, s, x, g, res, out, (long long)M, C, L, eps, fscale, fshift, film_bstride, (long long)ppi)
    if (need <= 1) IRSDE_LN(1, 4);
    else if (need <= 2) IRSDE_LN(2, 4);
    else if (need <= 4) IRSDE_LN(4, 2);
    else IRSDE_LN(8, 1);
#undef IRSDE_LN
    IRSDE_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------
// Full softmax attention (denoising-sde bottleneck) — module_util.py:182-204.  qkv: [B][N][384], out: [B][N][128].
// One wave = one 32-query tile of one (batch, head); flash-style loop over 32-key tiles on the fp32 MFMA pipe:
//   S^T = K Q^T   (A = K rows, B = Q^T; 16 x v_mfma_f32_32x32x2_f32)   -> lane (q = lane&31, half h) holds 16 of the 32 scores
//   online softmax over the keys of this query: 16 registers + one cross-half shuffle
//   O^T += V^T P^T (A = V rows straight from HBM, B = the lane's own P registers — the swapped product needs no transposition)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void full_attn_kernel(const float* __restrict__ qkv, float* __restrict__ out, const int N,
                                                        const float scale) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int bh = blockIdx.y, b = bh >> 2, head = bh & 3;
    const int q0 = (blockIdx.x * 4 + wave) * 32;
    if (q0 >= N) return;  // wave-uniform
    const float* base = qkv + (size_t)b * N * kQkv + head * kDh;
    const int q = q0 + l31;
    float qreg[16];
    {
        const float4* qp = reinterpret_cast<const float4*>(base + (size_t)(q < N ? q : q0) * kQkv + 16 * h);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const float4 t4 = qp[v];
            qreg[4 * v + 0] = t4.x * scale; qreg[4 * v + 1] = t4.y * scale;
            qreg[4 * v + 2] = t4.z * scale; qreg[4 * v + 3] = t4.w * scale;
        }
    }
    float m = -INFINITY, l = 0.f;
    floatx16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
    for (int j0 = 0; j0 < N; j0 += 32) {
        const int j = j0 + l31;
        float kreg[16];
        {
            const float4* kp = reinterpret_cast<const float4*>(base + (size_t)(j < N ? j : 0) * kQkv + kHid + 16 * h);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const float4 t4 = kp[v];
                kreg[4 * v + 0] = t4.x; kreg[4 * v + 1] = t4.y; kreg[4 * v + 2] = t4.z; kreg[4 * v + 3] = t4.w;
            }
        }
        float vreg[16];  // V[j0 + jj_h(s)][d = l31], jj_h(s) = (s&3) + 8(s>>2) + 4h  (the C-layout row of register s)
#pragma unroll
        for (int s2 = 0; s2 < 16; ++s2) {
            const int jj = j0 + (s2 & 3) + 8 * (s2 >> 2) + 4 * h;
            vreg[s2] = jj < N ? base[(size_t)jj * kQkv + 2 * kHid + l31] : 0.f;
        }
        floatx16 st;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
        for (int s2 = 0; s2 < 16; ++s2) st = __builtin_amdgcn_mfma_f32_32x32x2f32(kreg[s2], qreg[s2], st, 0, 0, 0);
        float tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int jj = j0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (jj >= N) st[r] = -INFINITY;
            tmax = fmaxf(tmax, st[r]);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float mnew = fmaxf(m, tmax);
        const float alpha = expf(m - mnew);
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            st[r] = expf(st[r] - mnew);
            psum += st[r];
        }
        psum += __shfl_xor(psum, 32, 64);
        l = l * alpha + psum;
        m = mnew;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] *= alpha;
#pragma unroll
        for (int s2 = 0; s2 < 16; ++s2) o = __builtin_amdgcn_mfma_f32_32x32x2f32(vreg[s2], st[s2], o, 0, 0, 0);
    }
    if (q < N) {
        const float il = 1.0f / l;
        float* op = out + ((size_t)b * N + q) * kHid + head * kDh;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4)  // registers 4g..4g+3 are d = 8g + 4h + {0..3}
            *reinterpret_cast<float4*>(op + 8 * g4 + 4 * h) =
                make_float4(o[4 * g4] * il, o[4 * g4 + 1] * il, o[4 * g4 + 2] * il, o[4 * g4 + 3] * il);
    }
}

// ---------------------------------------------------------------------------------------------
// Input prep: x0[b][y][x][0..P) over the physically zero-bordered (3 px) image, NCHW -> NHWC.
// ---------------------------------------------------------------------------------------------
__global__ void prep_input_kernel(const float* __restrict__ xt, const float* __restrict__ cond, float* __restrict__ x0,
                                  const int B, const int in_nc, const int P, const int H, const int W, const int Hp,
                                  const int Wp, const int reflect) {
    const int Hb = Hp + 6, Wb = Wp + 6;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)B * Hb * Wb;
    if (idx >= total) return;
    const int xb = (int)(idx % Wb);
    const size_t t1 = idx / Wb;
    const int yb = (int)(t1 % Hb);
    const int b = (int)(t1 / Hb);
    float v[16] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // in_nc <= 8
    const int y = yb - 3, x = xb - 3;
    // UNet: F.pad(..., 'reflect') to a multiple of 2^depth; NAFNet: zero pad (DenoisingNAFNet_arch.py:189-194)
    if (y >= 0 && y < Hp && x >= 0 && x < Wp && (reflect || (y < H && x < W))) {
        const int sy = y < H ? y : 2 * (H - 1) - y;  // F.pad(..., 'reflect') on the right/bottom
        const int sx = x < W ? x : 2 * (W - 1) - x;
        for (int c = 0; c < in_nc; ++c) {
            const size_t o = (((size_t)b * in_nc + c) * H + sy) * W + sx;
            if (cond) {
                const float cv = cond[o];
                v[c] = xt[o] - cv;
                v[in_nc + c] = cv;
            } else {
                v[c] = xt[o];  // denoising-sde variant: no condition input
            }
        }
    }
    float* op = x0 + idx * P;
    for (int c = 0; c < P; ++c) op[c] = v[c];
}

// ---------------------------------------------------------------------------------------------
// Time embedding path (rows = timesteps of the table, or batch items for tensor-valued t).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float act_apply(float v, int act) {
    if (act == ACT_SILU) return v / (1.0f + expf(-v));
    if (act == ACT_GELU) return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
    return v;
}

__global__ void sinusoid_kernel(const float* __restrict__ tvals, const float* __restrict__ freqs,
                                float* __restrict__ out, const int rows, const int half) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * half) return;
    const int r = idx / half, i = idx % half;
    const float a = tvals[r] * freqs[i];
    out[(size_t)r * 2 * half + i] = sinf(a);
    out[(size_t)r * 2 * half + half + i] = cosf(a);
}

// one wave per output feature; lanes stride the input dimension (coalesced weight row)
__global__ __launch_bounds__(256) void row_linear_kernel(const float* __restrict__ in, const int in_stride,
                                                         const float* __restrict__ W, const float* __restrict__ bias,
                                                         float* __restrict__ out, const int out_stride, const int rows,
                                                         const int in_dim, const int out_dim, const int act_in,
                                                         const int act_out) {
    const int lane = threadIdx.x & 63;
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= out_dim) return;
    const float* w = W + (size_t)o * in_dim;
    const float bo = bias ? bias[o] : 0.f;
    for (int r = 0; r < rows; ++r) {
        const float* x = in + (size_t)r * in_stride;
        float s = 0.f;
        for (int i = lane; i < in_dim; i += 64) s = fmaf(act_apply(x[i], act_in), w[i], s);
        s = wave_xor_sum(s, 64);
        if (lane == 0) out[(size_t)r * out_stride + o] = act_apply(s + bo, act_out);
    }
}

// One block (the step counter is read and advanced here: more blocks would race on it), 1024 threads, 16-byte pieces, 8 loads in flight per thread:
// the NAFNet FiLM row is 67 072 floats, and the 256-thread scalar loop this replaces took 104 us per step (profiles/r04_final_latent_bench_kernel_trace_stats.txt)
__global__ __launch_bounds__(1024) void step_begin_kernel(StepState* st, const float* __restrict__ film_table, const int film_row,
                                                          float* __restrict__ film_cur, const float* __restrict__ coef_table) {
    const int t = st->t_next;
    __syncthreads();
    const float* src = film_table + (size_t)t * film_row;
    if ((film_row & 3) == 0 && ((reinterpret_cast<size_t>(src) | reinterpret_cast<size_t>(film_cur)) & 15) == 0) {
        const int n4 = film_row >> 2;
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* d4 = reinterpret_cast<float4*>(film_cur);
        for (int i0 = threadIdx.x; i0 < n4; i0 += 8 * (int)blockDim.x) {
            float4 v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int i = i0 + j * (int)blockDim.x;
                v[j] = s4[i < n4 ? i : i0];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int i = i0 + j * (int)blockDim.x;
                if (i < n4) d4[i] = v[j];
            }
        }
    } else {
        for (int i = threadIdx.x; i < film_row; i += blockDim.x) film_cur[i] = src[i];
    }
    if (threadIdx.x < 12) st->coef[threadIdx.x] = coef_table[(size_t)t * 12 + threadIdx.x];
    if (threadIdx.x == 0) {
        st->t = t;
        st->t_next = t - 1;
    }
}

__global__ void set_step_kernel(StepState* st, const int t_next) {
    st->t = t_next;
    st->t_next = t_next;
}

// ---------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11) + Box-Muller.  counter = (quad, t, image, 0x1D5DE), key = seed.
// Keyed by the GLOBAL image index so results do not depend on how the batch is sharded over GPUs.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ __forceinline__ void philox_normal4(uint32_t quad, uint32_t t, uint32_t image, uint64_t seed, float z[4]) {
    uint32_t r[4];
    philox4x32_10(quad, t, image, 0x1D5DEu, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    const float s = 1.0f / 16777216.0f;
    const float u0 = ((float)(r[0] >> 8) + 0.5f) * s, u1 = ((float)(r[1] >> 8) + 0.5f) * s;
    const float u2 = ((float)(r[2] >> 8) + 0.5f) * s, u3 = ((float)(r[3] >> 8) + 0.5f) * s;
    const float ra = sqrtf(-2.0f * logf(u0)), rb = sqrtf(-2.0f * logf(u2));
    float sa, ca, sb, cb;
    sincosf(6.28318530717958647692f * u1, &sa, &ca);
    sincosf(6.28318530717958647692f * u3, &sb, &cb);
    z[0] = ra * ca; z[1] = ra * sa; z[2] = rb * cb; z[3] = rb * sb;
}

// coef row: [0] theta_t [1] sigma_t [2] sigma_bar_t [3] dt [4] sqrt(dt) [5] x0_gain=e^{Theta_t dt}
//           [6] posterior term1 [7] term2 [8] posterior std [9..11] unused
__global__ __launch_bounds__(256) void sde_update_kernel(const UpdateParams p) {
    const int b = blockIdx.y;
    const int CHW = p.C * p.H * p.W;
    const int HW = p.H * p.W;
    const int quad = blockIdx.x * blockDim.x + threadIdx.x;
    if (quad * 4 >= CHW) return;
    const int t = p.st ? p.st->t : p.t_imm;
    const float* cf = p.st ? p.st->coef : p.coef_imm;
    const float theta = cf[0], sigma = cf[1], sbar = cf[2], dt = cf[3];
    const float sqdt = cf[4], gain = cf[5], t1 = cf[6], t2 = cf[7];
    const float pstd = cf[8];
    int mode = p.mode;
    const float* noise = p.noise;
    long long noise_tstride = p.noise_tstride;
    unsigned long long seed = p.seed, image_offset = p.image_offset;
    if (p.ctl) {
        mode = p.ctl->mode; noise = p.ctl->noise; noise_tstride = p.ctl->noise_tstride;
        seed = p.ctl->seed; image_offset = p.ctl->image_offset;
    }
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    const bool need_z = mode != 1 && mode != 4;
    const int bg = b + p.batch0;   // index of this image in the call's batch (sub-batch plans: batch0 > 0)
    if (need_z && !noise) philox_normal4((uint32_t)quad, (uint32_t)t, (uint32_t)(image_offset + bg), seed, z);
    for (int k = 0; k < 4; ++k) {
        const int e = quad * 4 + k;
        if (e >= CHW) break;
        const size_t si = (size_t)b * CHW + e;
        const int c = e / HW, rem = e - c * HW, y = rem / p.W, xx = rem - y * p.W;
        const float eps_hat = p.pred[(size_t)b * p.sb + (size_t)c * p.sc + (size_t)y * p.sy + (size_t)xx * p.sx];
        const float x = p.x[si], mu = p.mu[si];
        if (need_z && noise) z[k] = noise[(size_t)t * noise_tstride + (size_t)bg * CHW + e];
        float xn;
        if (mode >= 3) {
            // DenoisingSDE (sde_utils.py:448-457, 44-48): mode 3 reverse_sde, mode 4 reverse_ode; cf[9] = exp(-2 Theta_t dt)
            const float score = -eps_hat / sbar;
            if (mode == 3) {
                const float drift = -0.5f * (sigma * sigma) * (1.0f + cf[9]) * score * dt;
                const float disp = sigma * (z[k] * sqdt);
                xn = x - drift - disp;
            } else {
                const float drift = -0.5f * (sigma * sigma) * cf[9] * score * dt;
                xn = x - drift;
            }
        } else if (mode == 2) {
            // sde_utils.py:237-239, 197-205, 219-223
            const float x0 = (x - mu - sbar * eps_hat) * gain + mu;
            const float mean = t1 * (x - mu) + t2 * (x0 - mu) + mu;
            xn = mean + pstd * z[k];
        } else {
            const float score = -eps_hat / sbar;  // sde_utils.py:184-185
            if (mode == 0) {
                const float drift = (theta * (mu - x) - sigma * sigma * score) * dt;  // :175-176
                const float disp = sigma * (z[k] * sqdt);                               // :181-182
                xn = x - drift - disp;                                                   // :44-45
            } else {
                const float drift = (theta * (mu - x) - 0.5f * (sigma * sigma) * score) * dt;  // :178-179
                xn = x - drift;                                                                  // :47-48
            }
        }
        p.x[si] = xn;
    }
}

__global__ void set_ctl_kernel(SampleCtl* ctl, const int mode, const float* noise, const long long noise_tstride,
                               const unsigned long long seed, const unsigned long long image_offset) {
    ctl->mode = mode; ctl->pad = 0; ctl->noise = noise; ctl->noise_tstride = noise_tstride;
    ctl->seed = seed; ctl->image_offset = image_offset;
}

__global__ void unpack_pred_kernel(const float* __restrict__ pred, float* __restrict__ out, const int B, const int C,
                                   const int H, const int W, const int Hp, const int Wp, const int stride) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)B * C * H * W;
    if (idx >= total) return;
    const int x = (int)(idx % W);
    size_t r = idx / W;
    const int y = (int)(r % H); r /= H;
    const int c = (int)(r % C);
    const int b = (int)(r / C);
    out[idx] = pred[(((size_t)b * Hp + y) * Wp + x) * stride + c];
}

template <typename T>
__global__ void nhwc_to_nchw_kernel(const T* __restrict__ in, float* __restrict__ out, const int B, const int C,
                                    const int H, const int W) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)B * C * H * W;
    if (idx >= total) return;
    const int x = (int)(idx % W);
    size_t r = idx / W;
    const int y = (int)(r % H); r /= H;
    const int c = (int)(r % C);
    const int b = (int)(r / C);
    out[idx] = ld1(in + (((size_t)b * H + y) * W + x) * C + c);
}

// ---------------------------------------------------------------------------------------------
// NAFNet (Refusion) — DenoisingNAFNet_arch.py:15-82
// depthwise 3x3 (+bias) -> SimpleGate, with per-tile channel sums for the SCA global average pool.
// Tile = kDwRows image rows x (pixel lanes x kDwRun) columns of one image; thread = (pixel lane, 4-channel group): the
// 2 x 9 depthwise weights of its channels live in registers, and the lane walks kDwRun columns to the right keeping a
// (kDwRows + 2) x 3 register window per gate half: one new window column = 6 rows x 2 halves of 16-byte loads yields
// kDwRows = 4 outputs, so every input row passes through the CU's L1 1.5 times (a one-row walk re-read it 3 times, and the
// kernel ran at the ~13 B/clk a CU can pull from L2, not at HBM speed).  Consecutive lanes = consecutive channel groups:
// each load instruction covers whole 128-byte lines.
// ---------------------------------------------------------------------------------------------
constexpr int kDwRows = 4;
constexpr int kDwRun = 16;

struct DwGeom {
    int gpp, PP, run, tiles_x, tiles_y;
};
static inline DwGeom dw_geom(int H, int W, int c) {
    DwGeom g;
    const int G = c >> 2;
    g.gpp = G < 256 ? G : 256;
    g.PP = 256 / g.gpp;
    // columns a lane walks: kDwRun, but no more than it takes the block's pixel lanes to cover the image width (r04: on the latent feature maps,
    // 64 .. 16 columns wide, a run of 16 left three of four lanes without work); at least 4, so that the two window columns a walk starts with stay < 50 % extra
    g.run = (W + g.PP - 1) / g.PP;
    g.run = g.run < 4 ? 4 : g.run > kDwRun ? kDwRun : g.run;
    g.tiles_x = (W + g.PP * g.run - 1) / (g.PP * g.run);
    g.tiles_y = (H + kDwRows - 1) / kDwRows;
    return g;
}

__device__ __forceinline__ float4 dw_widen(const float4 v) { return v; }
__device__ __forceinline__ float4 dw_widen(const f16x4 v) { return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]); }

// T = the storage type of u and out (fp32, or IEEE fp16 under IRSDE_FLAG_F16_ACT: the window loads widen, the gated product is rounded once on the store);
// the weights, the window, the accumulation and the per-tile sums — taken from the fp32 products, before the store rounding — are fp32 either way
template <typename T>
__global__ __launch_bounds__(256) void dwconv_gate_kernel(const T* __restrict__ u, const float* __restrict__ w,
                                                          const float* __restrict__ bias, T* __restrict__ out,
                                                          float* __restrict__ partial, const int H, const int W,
                                                          const int c, const int tiles_x, const int ntiles, const int run) {
    __shared__ float4 red[256];
    constexpr int R = kDwRows;
    using Win = std::conditional_t<std::is_same<T, float>::value, float4, f16x4>;   // a window entry: 4 channels as stored
    const int tile = blockIdx.x, b = blockIdx.y;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int HW = H * W;
    const int G = c >> 2;                        // float4 groups of gated channels
    const int gpp = G < 256 ? G : 256;           // groups handled per pass
    const int PP = 256 / gpp;                    // pixel lanes per pass
    const int C2 = 2 * c;
    for (int gc = 0; gc < G; gc += gpp) {
        const int g = gc + (int)(threadIdx.x % gpp);
        const int pl = threadIdx.x / gpp;
        float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
        const int y0 = ty * R, x0 = (tx * PP + pl) * run;
        if (g < G && pl < PP && x0 < W) {
            const int ch = g * 4;
            const float4 b1 = *reinterpret_cast<const float4*>(bias + ch);
            const float4 b2 = *reinterpret_cast<const float4*>(bias + c + ch);
            float4 w1[9], w2[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                w1[k] = *reinterpret_cast<const float4*>(w + k * C2 + ch);
                w2[k] = *reinterpret_cast<const float4*>(w + k * C2 + c + ch);
            }
            const T* ub = u + (size_t)b * HW * C2 + ch;
            // fp16 storage: the window holds the loaded halves as they are (half the registers of the fp32 window) and a tap widens its operand inside the
            // multiply-add.  (Widening at the load, inside the bounds branch, made every load wait for the one before: 1.6 x slower than the fp32 kernel.)
            const Win zero = {};
            auto ld = [&](int iy, int ix, int half) -> Win {
                if ((unsigned)iy >= (unsigned)H || (unsigned)ix >= (unsigned)W) return zero;
                return *reinterpret_cast<const Win*>(ub + ((size_t)iy * W + ix) * C2 + half * c);
            };
            Win win1[R + 2][3], win2[R + 2][3];  // [row y0 - 1 + r][column slot] of the two gate halves
            // one step: the new column x + 1 goes to slot CN (the oldest), the outputs of column x use slots (CL, CM, CN)
            auto step = [&](const int x, auto cl, auto cm, auto cn) {
                constexpr int CL = decltype(cl)::value, CM = decltype(cm)::value, CN = decltype(cn)::value;
#pragma unroll
                for (int r = 0; r < R + 2; ++r) {
                    win1[r][CN] = ld(y0 - 1 + r, x + 1, 0);
                    win2[r][CN] = ld(y0 - 1 + r, x + 1, 1);
                }
#pragma unroll
                for (int ro = 0; ro < R; ++ro) {
                    const int y = y0 + ro;
                    if (y >= H) break;
                    float4 a1 = b1, a2 = b2;
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky) {
                        const int slot[3] = {CL, CM, CN};
#pragma unroll
                        for (int kx = 0; kx < 3; ++kx) {
                            const float4 v1 = dw_widen(win1[ro + ky][slot[kx]]), v2 = dw_widen(win2[ro + ky][slot[kx]]);
                            const float4 q1 = w1[ky * 3 + kx], q2 = w2[ky * 3 + kx];
                            a1.x = fmaf(v1.x, q1.x, a1.x); a1.y = fmaf(v1.y, q1.y, a1.y);
                            a1.z = fmaf(v1.z, q1.z, a1.z); a1.w = fmaf(v1.w, q1.w, a1.w);
                            a2.x = fmaf(v2.x, q2.x, a2.x); a2.y = fmaf(v2.y, q2.y, a2.y);
                            a2.z = fmaf(v2.z, q2.z, a2.z); a2.w = fmaf(v2.w, q2.w, a2.w);
                        }
                    }
                    const float4 o = make_float4(a1.x * a2.x, a1.y * a2.y, a1.z * a2.z, a1.w * a2.w);
                    st4(out + ((size_t)b * HW + (size_t)y * W + x) * c + ch, o);
                    sum.x += o.x; sum.y += o.y; sum.z += o.z; sum.w += o.w;
                }
            };
#pragma unroll
            for (int r = 0; r < R + 2; ++r) {  // columns x0 - 1 and x0 into slots 0 and 1: the first step loads slot 2
                win1[r][0] = ld(y0 - 1 + r, x0 - 1, 0); win2[r][0] = ld(y0 - 1 + r, x0 - 1, 1);
                win1[r][1] = ld(y0 - 1 + r, x0, 0);     win2[r][1] = ld(y0 - 1 + r, x0, 1);
            }
            using I0 = std::integral_constant<int, 0>;
            using I1 = std::integral_constant<int, 1>;
            using I2 = std::integral_constant<int, 2>;
            const int xe = x0 + run < W ? x0 + run : W;
            for (int x = x0; x < xe; x += 3) {  // three steps per iteration: the slot roles rotate at compile time
                step(x, I0{}, I1{}, I2{});
                if (x + 1 < xe) step(x + 1, I1{}, I2{}, I0{});
                if (x + 2 < xe) step(x + 2, I2{}, I0{}, I1{});
            }
        }
        red[threadIdx.x] = sum;
        __syncthreads();
        if (pl == 0 && g < G) {  // fixed-order reduction over the pixel lanes: deterministic
            float4 t = red[threadIdx.x];
            for (int q = 1; q < PP; ++q) {
                const float4 r = red[threadIdx.x + q * gpp];
                t.x += r.x; t.y += r.y; t.z += r.z; t.w += r.w;
            }
            *reinterpret_cast<float4*>(partial + ((size_t)b * ntiles + tile) * c + g * 4) = t;
        }
        __syncthreads();
    }
}

// mean[b][k] = sum_tiles partial / HW  (second stage of the deterministic global average pool)
__global__ __launch_bounds__(256) void sca_mean_kernel(const float* __restrict__ partial, const int ntiles,
                                                       float* __restrict__ mean, const int c, const float inv_hw) {
    __shared__ float red[256];
    const int b = blockIdx.y;
    const int k = blockIdx.x * 64 + (threadIdx.x & 63);
    const int tl = threadIdx.x >> 6;
    float t = 0.f;
    if (k < c)
        for (int q = tl; q < ntiles; q += 4) t += partial[((size_t)b * ntiles + q) * c + k];
    red[threadIdx.x] = t;
    __syncthreads();
    if (tl == 0 && k < c) mean[(size_t)b * c + k] = ((red[threadIdx.x] + red[threadIdx.x + 64]) + (red[threadIdx.x + 128] + red[threadIdx.x + 192])) * inv_hw;
}

// s[b][o] = bias[o] + sum_k W[o][k] * mean[b][k]   (AdaptiveAvgPool2d(1) -> 1x1 conv, DenoisingNAFNet_arch.py:29-33)
// r06: both steps in one launch for the small feature maps (the latent network's levels: every launch there costs ~5 us whatever it does, profiles/r06_notes.md 3b).
// Every block sums the image's tile partials itself — the same four strided partial sums and the same order as sca_mean_kernel: the same bits — and
// computes four output channels.
__global__ __launch_bounds__(256) void sca_fused_kernel(const float* __restrict__ partial, const int ntiles, const float* __restrict__ W,
                                                        const float* __restrict__ bias, float* __restrict__ s_out, const int c, const float inv_hw) {
    extern __shared__ float sca_mean_lds[];
    const int b = blockIdx.y;
    for (int k = threadIdx.x; k < c; k += 256) {
        float t[4] = {0.f, 0.f, 0.f, 0.f};
        for (int q0 = 0; q0 < ntiles; q0 += 4)
#pragma unroll
            for (int tl = 0; tl < 4; ++tl)
                if (q0 + tl < ntiles) t[tl] += partial[((size_t)b * ntiles + q0 + tl) * c + k];
        sca_mean_lds[k] = ((t[0] + t[1]) + (t[2] + t[3])) * inv_hw;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= c) return;
    const float* wr = W + (size_t)o * c;
    float t = 0.f;
    for (int k = lane; k < c; k += 64) t = fmaf(wr[k], sca_mean_lds[k], t);
    t = wave_xor_sum(t, 64);
    if (lane == 0) s_out[(size_t)b * c + o] = t + bias[o];
}
__global__ __launch_bounds__(256) void sca_kernel(const float* __restrict__ mean, const float* __restrict__ W,
                                                  const float* __restrict__ bias, float* __restrict__ s_out, const int c) {
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= c) return;
    const float* wr = W + (size_t)o * c;
    const float* mb = mean + (size_t)b * c;
    float t = 0.f;
    for (int k = lane; k < c; k += 64) t = fmaf(wr[k], mb[k], t);
    t = wave_xor_sum(t, 64);
    if (lane == 0) s_out[(size_t)b * c + o] = t + bias[o];
}

// ---------------------------------------------------------------------------------------------
// r06: NAFBlock norm1 + conv1 / norm2 + conv4 as ONE launch on the small-channel levels of the fp16 operand mode (c = 64 / 128 / 256: the latent network outside
// the chain): LayerNorm + time FiLM (DenoisingNAFNet_arch.py:63-64,74-75) of a 64-pixel tile straight into the fp16 A operand in LDS, the whole K = c in one
// piece (no K loop, every load of the tile in flight at once), v_mfma_f32_32x32x16_f16 against a 64-column weight tile, then bias (conv1) or bias + SimpleGate
// (+ lens FiLM) (conv4).  Why: at these sizes a launch costs ~5 us whatever it does and the two-kernel form pays three or four serialised memory latencies
// (profiles/r06_notes.md 3b).  The LayerNorm arithmetic is layernorm_kernel's (KV = 1: L = c / 4 lanes per pixel, one float4 each, the same summation order,
// this file is compiled without FMA contraction) and the rounding to fp16 is the consuming convolution's: the same operand bits as the two-kernel path.
// ---------------------------------------------------------------------------------------------
struct NafLnConvArgs {
    const float* x;          // [M][c] fp32
    const float* g;          // LayerNorm gain [c]
    const float* fscale;     // FiLM rows (row of image b at + b * film_bstride)
    const float* fshift;
    int film_bstride;
    long long ppi;           // pixels per image
    const unsigned short* w; // fp16 [Cout][c]
    const float* bias;       // [Cout]
    float* out;              // [M][Cout] or (gate) [M][Cout / 2]
    const float* gate_film;  // gate only: per-image [scale (Cout / 2) | shift (Cout / 2)] or nullptr
    int gate_film_bstride;
    int gate;
    int M, Cout;
    // PRO 1 / 2 (conv3 / conv5: no LayerNorm): the A operand is x itself, PRO 1 times the per-image channel scale in_scale[b][c] (SCA, :68) before the rounding;
    // epilogue out = res + (acc + bias) * ch_scale (beta / gamma, :70,81)
    const float* in_scale;
    const float* ch_scale;
    const float* res;
};

// PRO: 0 LayerNorm + FiLM, 1 per-image channel scale, 2 plain
// T: the storage type of x, res and out (fp32, or IEEE fp16 under IRSDE_FLAG_F16_ACT: behind the float pointers of the argument block); the lane layout, the fp32
// LayerNorm arithmetic and its summation order are the same for both, the epilogues round once on the store
template <int C, int PRO = 0, typename T = float>
__global__ __launch_bounds__(256, 2) void naf_lnconv_kernel(const NafLnConvArgs a) {
    const T* const xT = reinterpret_cast<const T*>(a.x);
    const T* const resT = reinterpret_cast<const T*>(a.res);
    T* const outT = reinterpret_cast<T*>(a.out);
    constexpr int L = C / 4;                 // lanes per pixel (16 / 32 / 64)
    constexpr int RPP = 256 / L;             // pixels per pass of the block
    constexpr int NPASS = 64 / RPP;          // passes (4 / 8 / 16): one float4 per lane and pass
    constexpr int ROWB = C * 2 + 16;         // LDS row stride (bytes): K halves + 16-byte pad (conflict-free 16-byte fragment reads)
    extern __shared__ __attribute__((aligned(16))) char lnc_lds[];
    char* As = lnc_lds;                      // [64 pixels][ROWB]
    char* Bs = lnc_lds + 64 * ROWB;          // [64 output channels][ROWB]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nblk_n = a.Cout / 64;
    // XCD-aware remap: the column tiles of a pixel tile run back to back on one XCD (they share the pixel tile in L2)
    int wgid;
    {
        const int orig = blockIdx.x, nwg = gridDim.x;
        const int xcd = orig & 7, q = nwg >> 3, r = nwg & 7;
        wgid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
    }
    const int mblk = wgid / nblk_n, nblk = wgid - mblk * nblk_n;
    const int m0 = mblk * 64, n0 = nblk * 64;
    // ---- every load of the tile first: the pixel rows, the weight tile, the LayerNorm / FiLM vectors ----
    const int li = tid % L, sub = tid / L;
    float4 v[NPASS];
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps) {
        const int m = m0 + ps * RPP + sub;
        v[ps] = ld4(xT + (size_t)(m < a.M ? m : a.M - 1) * C + 4 * li);
    }
    constexpr int BCH = (64 * C * 2 / 16) / 256;   // 16-byte chunks of the weight tile per thread (2 / 4 / 8)
    floatx4 wv[BCH];
#pragma unroll
    for (int i = 0; i < BCH; ++i) {
        const int idx = tid + 256 * i, row = idx / (C / 8), ch = idx % (C / 8);
        wv[i] = *reinterpret_cast<const floatx4*>(reinterpret_cast<const char*>(a.w) + ((size_t)(n0 + row) * C) * 2 + ch * 16);
    }
    float4 gg = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (PRO == 0) gg = reinterpret_cast<const float4*>(a.g)[li];
#pragma unroll
    for (int i = 0; i < BCH; ++i) {
        const int idx = tid + 256 * i, row = idx / (C / 8), ch = idx % (C / 8);
        *reinterpret_cast<floatx4*>(Bs + row * ROWB + ch * 16) = wv[i];
    }
    // ---- LayerNorm + FiLM of the 64 pixels (layernorm_kernel, KV = 1), rounded to fp16 into the A tile ----
    const float invC = 1.0f / (float)C;
    if constexpr (PRO != 0) {
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) {
            floatx4 f = {v[ps].x, v[ps].y, v[ps].z, v[ps].w};
            if constexpr (PRO == 1) {   // (conv_igemm's INSCALE staging: fp32 product, then the rounding)
                const int m = m0 + ps * RPP + sub;
                const float4 sc = *reinterpret_cast<const float4*>(a.in_scale + (size_t)((m < a.M ? m : a.M - 1) / a.ppi) * C + 4 * li);
                f = f * floatx4{sc.x, sc.y, sc.z, sc.w};
            }
            *reinterpret_cast<f16x4*>(As + (ps * RPP + sub) * ROWB + li * 8) = __builtin_convertvector(f, f16x4);
        }
    } else
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps) {
        const int m = m0 + ps * RPP + sub;
        float s = (v[ps].x + v[ps].y) + (v[ps].z + v[ps].w);
        for (int o = L >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        const float mean = s * invC;
        float4 d = v[ps];
        d.x -= mean; d.y -= mean; d.z -= mean; d.w -= mean;
        float q = (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
        for (int o = L >> 1; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
        const float rstd = 1.0f / sqrtf(q * invC + 1e-5f);
        const size_t frow = (size_t)(a.film_bstride ? (m < a.M ? m : a.M - 1) / a.ppi : 0) * a.film_bstride;
        const float4 s4 = reinterpret_cast<const float4*>(a.fscale + frow)[li];
        const float4 h4 = reinterpret_cast<const float4*>(a.fshift + frow)[li];
        float4 o4;
        o4.x = d.x * rstd * gg.x; o4.y = d.y * rstd * gg.y; o4.z = d.z * rstd * gg.z; o4.w = d.w * rstd * gg.w;
        o4.x = o4.x * (s4.x + 1.0f) + h4.x; o4.y = o4.y * (s4.y + 1.0f) + h4.y;
        o4.z = o4.z * (s4.z + 1.0f) + h4.z; o4.w = o4.w * (s4.w + 1.0f) + h4.w;
        const floatx4 f = {o4.x, o4.y, o4.z, o4.w};
        *reinterpret_cast<f16x4*>(As + (ps * RPP + sub) * ROWB + li * 8) = __builtin_convertvector(f, f16x4);
    }
    __syncthreads();
    // ---- 64 x 64 x C on the matrix pipe: wave (wm, wn) owns a 32 x 32 tile ----
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, h = lane >> 5;
    floatx16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const char* ap = As + (wm * 32 + l31) * ROWB + h * 16;
    const char* bp = Bs + (wn * 32 + l31) * ROWB + h * 16;
#pragma unroll
    for (int ks = 0; ks < C / 16; ++ks)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16x8*>(ap + ks * 32), *reinterpret_cast<const f16x8*>(bp + ks * 32), acc, 0, 0, 0);
    // ---- epilogue: acc[r] = row 8 (r >> 2) + 4 h + (r & 3), column l31 of the wave's tile ----
    const int n = n0 + wn * 32 + l31;
    const float bn = a.bias[n];
    if constexpr (PRO != 0) {   // out = res + (acc + bias) * ch_scale
        const float cs = a.ch_scale[n];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm * 32 + 8 * (r >> 2) + 4 * h + (r & 3);
            if (m < a.M) {
                float t = (acc[r] + bn) * cs;
                t += ld1(resT + (size_t)m * a.Cout + n);
                st1(outT + (size_t)m * a.Cout + n, t);
            }
        }
    } else if (!a.gate) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm * 32 + 8 * (r >> 2) + 4 * h + (r & 3);
            if (m < a.M) st1(outT + (size_t)m * a.Cout + n, acc[r] + bn);
        }
    } else {   // SimpleGate: the packed weight rows pair columns (2 j, 2 j + 1); product j, then the per-image lens FiLM
        const int ch = a.Cout >> 1, oc = n >> 1;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm * 32 + 8 * (r >> 2) + 4 * h + (r & 3);
            const float t = acc[r] + bn;
            const float other = __shfl_xor(t, 1, 64);
            float gv = (lane & 1) ? other * t : t * other;   // v[2 j] * v[2 j + 1]
            if (a.gate_film) {
                const float* f = a.gate_film + (size_t)((m < a.M ? m : a.M - 1) / a.ppi) * a.gate_film_bstride;
                gv = gv * (f[oc] + 1.0f) + f[ch + oc];
            }
            if (!(lane & 1) && m < a.M) st1(outT + (size_t)m * ch + oc, gv);
        }
    }
}

__global__ void row_gate_kernel(const float* __restrict__ in, float* __restrict__ out, const int rows, const int h) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * h) return;
    const int r = idx / h, j = idx - r * h;
    out[idx] = in[(size_t)r * 2 * h + j] * in[(size_t)r * 2 * h + h + j];
}

__global__ void fill_random_kernel(float* p, const size_t n, const unsigned seed, const float scale) {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q * 4 >= n) return;
    float z[4];
    philox_normal4((uint32_t)q, (uint32_t)(q >> 32), seed, 0x5EEDULL, z);
    for (int k = 0; k < 4; ++k)
        if (q * 4 + k < n) p[q * 4 + k] = z[k] * scale;
}

__global__ void philox_normal_kernel(float* out, const int CHW, const int t, const uint64_t seed,
                                     const uint64_t image_offset) {
    const int b = blockIdx.y;
    const int quad = blockIdx.x * blockDim.x + threadIdx.x;
    if (quad * 4 >= CHW) return;
    float z[4];
    philox_normal4((uint32_t)quad, (uint32_t)t, (uint32_t)(image_offset + b), seed, z);
    for (int k = 0; k < 4; ++k)
        if (quad * 4 + k < CHW) out[(size_t)b * CHW + quad * 4 + k] = z[k];
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// Launchers
// ---------------------------------------------------------------------------------------------
void launch_layernorm(const float* x, const float* g, const float* res, float* out, int64_t M, int C, float eps,
                      hipStream_t s, bool bf16) {
    if (bf16)
        launch_ln_t(reinterpret_cast<const bf16_t*>(x), g, reinterpret_cast<const bf16_t*>(res), reinterpret_cast<bf16_t*>(out), M,
                    C, eps, nullptr, nullptr, 0, 1, s);
    else
        launch_ln_t(x, g, res, out, M, C, eps, nullptr, nullptr, 0, 1, s);
}

void launch_layernorm_film(const float* x, const float* g, const float* scale, const float* shift, int film_bstride,
                           int64_t pixels_per_image, float* out, int64_t M, int C, float eps, hipStream_t s, bool f16) {
    if (f16)
        launch_ln_t(reinterpret_cast<const f16_t*>(x), g, (const f16_t*)nullptr, reinterpret_cast<f16_t*>(out), M, C, eps, scale, shift, film_bstride,
                    pixels_per_image, s);
    else
        launch_ln_t(x, g, (const float*)nullptr, out, M, C, eps, scale, shift, film_bstride, pixels_per_image, s);
}

int dwgate_tiles(int H, int W, int c) {
    const DwGeom g = dw_geom(H, W, c);
    return g.tiles_x * g.tiles_y;
}

bool naf_lnconv_ok(int c, int Cout, long long M) { return (c == 64 || c == 128 || c == 256) && Cout % 64 == 0 && M > 0 && M < (1ll << 31); }

void naf_lnconv_global_init() {
    IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(naf_lnconv_kernel<64>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(naf_lnconv_kernel<128>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(naf_lnconv_kernel<256>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(naf_lnconv_kernel<256, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(naf_lnconv_kernel<256, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(naf_lnconv_kernel<256, 0, f16_t>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(naf_lnconv_kernel<256, 1, f16_t>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    IRSDE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(naf_lnconv_kernel<256, 2, f16_t>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
}

// norm + FiLM + 1x1 convolution (fp16 operands: w16 = the layer's fp16 weight copy [Cout][c]) in one launch; gate: SimpleGate epilogue (+ gate_film)
void launch_naf_lnconv(const float* x, const float* g, const float* fscale, const float* fshift, int film_bstride, int64_t pixels_per_image,
                       const unsigned short* w16, const float* bias, float* out, int64_t M, int c, int Cout, int gate, const float* gate_film,
                       int gate_film_bstride, hipStream_t s, bool f16) {
    if (!naf_lnconv_ok(c, Cout, M)) throw HipError("naf_lnconv: unsupported shape");
    NafLnConvArgs a;
    a.x = x; a.g = g; a.fscale = fscale; a.fshift = fshift; a.film_bstride = film_bstride; a.ppi = pixels_per_image;
    a.w = w16; a.bias = bias; a.out = out; a.gate_film = gate_film; a.gate_film_bstride = gate_film_bstride; a.gate = gate;
    a.M = (int)M; a.Cout = Cout;
    a.in_scale = nullptr; a.ch_scale = nullptr; a.res = nullptr;
    const dim3 grid((unsigned)(((M + 63) / 64) * (Cout / 64)));
    const size_t lds = (size_t)128 * (c * 2 + 16);
    if (f16) {
        if (c == 64) hipLaunchKernelGGL((naf_lnconv_kernel<64, 0, f16_t>), grid, dim3(256), lds, s, a);
        else if (c == 128) hipLaunchKernelGGL((naf_lnconv_kernel<128, 0, f16_t>), grid, dim3(256), lds, s, a);
        else hipLaunchKernelGGL((naf_lnconv_kernel<256, 0, f16_t>), grid, dim3(256), lds, s, a);
    } else if (c == 64) hipLaunchKernelGGL(naf_lnconv_kernel<64>, grid, dim3(256), lds, s, a);
    else if (c == 128) hipLaunchKernelGGL(naf_lnconv_kernel<128>, grid, dim3(256), lds, s, a);
    else hipLaunchKernelGGL(naf_lnconv_kernel<256>, grid, dim3(256), lds, s, a);
    IRSDE_HIP_CHECK(hipGetLastError());
}

// conv3 / conv5 of a NAFBlock on the same kernel: out = res + (W (x * in_scale) + bias) * ch_scale, in_scale (per image and input channel) optional
void launch_naf_pwconv(const float* x, const float* in_scale, int64_t pixels_per_image, const unsigned short* w16, const float* bias, const float* ch_scale,
                       const float* res, float* out, int64_t M, int c, int Cout, hipStream_t s, bool f16) {
    if (!naf_lnconv_ok(c, Cout, M) || !ch_scale || !res) throw HipError("naf_pwconv: unsupported shape");
    NafLnConvArgs a;
    a.x = x; a.g = nullptr; a.fscale = nullptr; a.fshift = nullptr; a.film_bstride = 0; a.ppi = pixels_per_image;
    a.w = w16; a.bias = bias; a.out = out; a.gate_film = nullptr; a.gate_film_bstride = 0; a.gate = 0;
    a.M = (int)M; a.Cout = Cout;
    a.in_scale = in_scale; a.ch_scale = ch_scale; a.res = res;
    const dim3 grid((unsigned)(((M + 63) / 64) * (Cout / 64)));
    const size_t lds = (size_t)128 * (c * 2 + 16);
#define IRSDE_PW(CC, TT) do { if (in_scale) hipLaunchKernelGGL((naf_lnconv_kernel<CC, 1, TT>), grid, dim3(256), lds, s, a); else hipLaunchKernelGGL((naf_lnconv_kernel<CC, 2, TT>), grid, dim3(256), lds, s, a); } while (0)
    if (f16) {
        if (c == 64) IRSDE_PW(64, f16_t); else if (c == 128) IRSDE_PW(128, f16_t); else IRSDE_PW(256, f16_t);
    } else {
        if (c == 64) IRSDE_PW(64, float); else if (c == 128) IRSDE_PW(128, float); else IRSDE_PW(256, float);
    }
#undef IRSDE_PW
    IRSDE_HIP_CHECK(hipGetLastError());
}

void launch_dwconv_gate(const float* u, const float* w, const float* bias, float* out, float* partial, int B, int H, int W,
                        int c, hipStream_t s, bool f16) {
    if (c % 4) throw HipError("dwconv_gate: channel count must be a multiple of 4");
    const DwGeom g = dw_geom(H, W, c);
    const int nt = g.tiles_x * g.tiles_y;
    if (f16)
        hipLaunchKernelGGL(dwconv_gate_kernel<f16_t>, dim3(nt, B), dim3(256), 0, s, reinterpret_cast<const f16_t*>(u), w, bias, reinterpret_cast<f16_t*>(out), partial,
                           H, W, c, g.tiles_x, nt, g.run);
    else
        hipLaunchKernelGGL(dwconv_gate_kernel<float>, dim3(nt, B), dim3(256), 0, s, u, w, bias, out, partial, H, W, c, g.tiles_x, nt, g.run);
    IRSDE_HIP_CHECK(hipGetLastError());
}

void launch_sca(const float* partial, int ntiles, const float* W, const float* bias, float* mean, float* s_out, int B,
                int c, int HW, hipStream_t s) {
    if ((long long)ntiles * c <= 65536 && c <= 4096) {   // small maps: one launch (every block re-sums <= 256 KB of partials from L2)
        hipLaunchKernelGGL(sca_fused_kernel, dim3((c + 3) / 4, B), dim3(256), (size_t)c * 4, s, partial, ntiles, W, bias, s_out, c, 1.0f / (float)HW);
    } else {
        launch_sca_mean(partial, ntiles, mean, B, c, HW, s);
        hipLaunchKernelGGL(sca_kernel, dim3((c + 3) / 4, B), dim3(256), 0, s, mean, W, bias, s_out, c);
    }
    IRSDE_HIP_CHECK(hipGetLastError());
}

void launch_sca_mean(const float* partial, int ntiles, float* mean, int B, int c, int HW, hipStream_t s) {
    hipLaunchKernelGGL(sca_mean_kernel, dim3((c + 63) / 64, B), dim3(256), 0, s, partial, ntiles, mean, c, 1.0f / (float)HW);
    IRSDE_HIP_CHECK(hipGetLastError());
}

void launch_row_gate(const float* in, float* out, int rows, int h, hipStream_t s) {
    const int total = rows * h;
    hipLaunchKernelGGL(row_gate_kernel, dim3((total + 255) / 256), dim3(256), 0, s, in, out, rows, h);
    IRSDE_HIP_CHECK(hipGetLastError());
}

void launch_full_attention(const float* qkv, float* out, int B, int N, hipStream_t s) {
    const int qtiles = (N + 31) / 32;
    hipLaunchKernelGGL(full_attn_kernel, dim3((qtiles + 3) / 4, B * kHeads), dim3(256), 0, s, qkv, out, N,
                       1.0f / sqrtf((float)kDh));
    IRSDE_HIP_CHECK(hipGetLastError());
}

void launch_prep_input(const float* xt, const float* cond, float* x0, int B, int in_nc, int H, int W, int Hp, int Wp,
                       hipStream_t s, int reflect) {
    const int P = ((cond ? 2 : 1) * in_nc + 3) & ~3;
    if (P > 16) throw HipError("prep_input: more than 8 (conditional) / 16 (unconditional) input channels unsupported");
    const size_t total = (size_t)B * (Hp + 6) * (Wp + 6);
    hipLaunchKernelGGL(prep_input_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, xt, cond, x0, B,
                       in_nc, P, H, W, Hp, Wp, reflect);
    IRSDE_HIP_CHECK(hipGetLastError());
}

void launch_sinusoid(const float* tvals, const float* freqs, float* out, int rows, int half, hipStream_t s) {
    const int total = rows * half;
    hipLaunchKernelGGL(sinusoid_kernel, dim3((total + 255) / 256), dim3(256), 0, s, tvals, freqs, out, rows, half);
    IRSDE_HIP_CHECK(hipGetLastError());
}

void launch_row_linear(const float* in, int in_stride, const float* W, const float* b, float* out, int out_stride,
                       int rows, int in_dim, int out_dim, int act_in, int act_out, hipStream_t s) {
    hipLaunchKernelGGL(row_linear_kernel, dim3((out_dim + 3) / 4), dim3(256), 0, s, in, in_stride, W, b, out,
                       out_stride, rows, in_dim, out_dim, act_in, act_out);
    IRSDE_HIP_CHECK(hipGetLastError());
}

void launch_step_begin(StepState* st, const float* film_table, int film_row, float* film_cur, const float* coef_table,
                       hipStream_t s) {
    hipLaunchKernelGGL(step_begin_kernel, dim3(1), dim3(1024), 0, s, st, film_table, film_row, film_cur, coef_table);
    IRSDE_HIP_CHECK(hipGetLastError());
}

void launch_set_step(StepState* st, int t_next, hipStream_t s) {
    hipLaunchKernelGGL(set_step_kernel, dim3(1), dim3(1), 0, s, st, t_next);
    IRSDE_HIP_CHECK(hipGetLastError());
}

void launch_sde_update(const UpdateParams& p, hipStream_t s) {
    const int CHW = p.C * p.H * p.W;
    const int quads = (CHW + 3) / 4;
    hipLaunchKernelGGL(sde_update_kernel, dim3((quads + 255) / 256, p.B), dim3(256), 0, s, p);
    IRSDE_HIP_CHECK(hipGetLastError());
}

void launch_set_ctl(SampleCtl* ctl, int mode, const float* noise, long long noise_tstride, unsigned long long seed,
                    unsigned long long image_offset, hipStream_t s) {
    hipLaunchKernelGGL(set_ctl_kernel, dim3(1), dim3(1), 0, s, ctl, mode, noise, noise_tstride, seed, image_offset);
    IRSDE_HIP_CHECK(hipGetLastError());
}

void launch_unpack_pred(const float* pred, float* out, int B, int C, int H, int W, int Hp, int Wp, int stride, hipStream_t s) {
    const size_t total = (size_t)B * C * H * W;
    hipLaunchKernelGGL(unpack_pred_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, pred, out, B, C, H,
                       W, Hp, Wp, stride);
    IRSDE_HIP_CHECK(hipGetLastError());
}

void launch_nhwc_to_nchw(const float* in, float* out, int B, int C, int H, int W, hipStream_t s, bool bf16, bool f16) {
    const size_t total = (size_t)B * C * H * W;
    if (f16)
        hipLaunchKernelGGL(nhwc_to_nchw_kernel<f16_t>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                           reinterpret_cast<const f16_t*>(in), out, B, C, H, W);
    else if (bf16)
        hipLaunchKernelGGL(nhwc_to_nchw_kernel<bf16_t>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                           reinterpret_cast<const bf16_t*>(in), out, B, C, H, W);
    else
        hipLaunchKernelGGL(nhwc_to_nchw_kernel<float>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, in, out, B, C, H,
                           W);
    IRSDE_HIP_CHECK(hipGetLastError());
}

void launch_fill_random(float* p, size_t n, unsigned seed, float scale, hipStream_t s) {
    const size_t quads = (n + 3) / 4;
    hipLaunchKernelGGL(fill_random_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, s, p, n, seed, scale);
    IRSDE_HIP_CHECK(hipGetLastError());
}

void launch_philox_normal(float* out, int B, int CHW, int t, uint64_t seed, uint64_t image_offset, hipStream_t s) {
    const int quads = (CHW + 3) / 4;
    hipLaunchKernelGGL(philox_normal_kernel, dim3((quads + 255) / 256, B), dim3(256), 0, s, out, CHW, t, seed,
                       image_offset);
    IRSDE_HIP_CHECK(hipGetLastError());
}

__global__ void bf16_to_f32_kernel(const bf16_t* __restrict__ in, float* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (float)in[i];
}
void launch_bf16_to_f32(const unsigned short* in, float* out, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(bf16_to_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const bf16_t*>(in), out, n);
    IRSDE_HIP_CHECK(hipGetLastError());
}

__global__ void f16_to_f32_kernel(const _Float16* __restrict__ in, float* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (float)in[i];
}
void launch_f16_to_f32(const unsigned short* in, float* out, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(f16_to_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const _Float16*>(in), out, n);
    IRSDE_HIP_CHECK(hipGetLastError());
}

// out = a + b (latent NAFNet: ending(x + intro); latent UNet: final_conv(x + h[0]))
__global__ void add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, size_t n4) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const float4 x = reinterpret_cast<const float4*>(a)[i], y = reinterpret_cast<const float4*>(b)[i];
    reinterpret_cast<float4*>(out)[i] = make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
}
void launch_add(const float* a, const float* b, float* out, size_t n, hipStream_t s) {
    if (n % 4) throw HipError("launch_add: element count must be a multiple of 4");
    hipLaunchKernelGGL(add_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, s, a, b, out, n / 4);
    IRSDE_HIP_CHECK(hipGetLastError());
}

// NCHW [B][C][H][W] -> NHWC [B][Hp][Wp][Cp]: channels >= C are zero; rows/cols >= H/W are reflect-padded (reflect=1,
// F.pad 'reflect' on the right/bottom) or zero
__global__ void nchw_to_nhwc_pad_kernel(const float* __restrict__ in, float* __restrict__ out, const int B, const int C,
                                        const int H, const int W, const int Hp, const int Wp, const int Cp, const int reflect) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)B * Hp * Wp * Cp;
    if (idx >= total) return;
    const int c = (int)(idx % Cp);
    size_t r = idx / Cp;
    const int x = (int)(r % Wp); r /= Wp;
    const int y = (int)(r % Hp);
    const int b = (int)(r / Hp);
    float v = 0.f;
    if (c < C && (reflect || (y < H && x < W))) {
        const int sy = y < H ? y : 2 * (H - 1) - y, sx = x < W ? x : 2 * (W - 1) - x;
        v = in[(((size_t)b * C + c) * H + sy) * W + sx];
    }
    out[idx] = v;
}
void launch_nchw_to_nhwc_pad(const float* in, float* out, int B, int C, int H, int W, int Hp, int Wp, int Cp, int reflect,
                             hipStream_t s) {
    const size_t total = (size_t)B * Hp * Wp * Cp;
    hipLaunchKernelGGL(nchw_to_nhwc_pad_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, in, out, B, C, H, W, Hp,
                       Wp, Cp, reflect);
    IRSDE_HIP_CHECK(hipGetLastError());
}

// fp32 -> bf16 (round to nearest even) copy of packed conv weights for the bf16-MFMA mode
__global__ void f32_to_bf16_kernel(const float* __restrict__ in, unsigned short* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const __bf16 b = (__bf16)in[i];
    out[i] = __builtin_bit_cast(unsigned short, b);
}
void launch_f32_to_bf16(const float* in, unsigned short* out, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(f32_to_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, out, n);
    IRSDE_HIP_CHECK(hipGetLastError());
}

// fp32 -> IEEE fp16 (round to nearest even) copy of packed conv weights for the fp16-MFMA mode (IRSDE_FLAG_FP16)
__global__ void f32_to_f16_kernel(const float* __restrict__ in, unsigned short* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const _Float16 b = (_Float16)in[i];
    out[i] = __builtin_bit_cast(unsigned short, b);
}
void launch_f32_to_f16(const float* in, unsigned short* out, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(f32_to_f16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, out, n);
    IRSDE_HIP_CHECK(hipGetLastError());
}

}  // namespace irsde
