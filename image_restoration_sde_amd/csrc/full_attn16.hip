// Full softmax attention on bf16 tensors for gfx950 (wave64): the denoising-sde bottleneck under IRSDE_FLAG_BF16_ACT — module_util.py:193-204.
//   qkv bf16 [B][N][384] (rows q | k | v, 4 heads x 32)  ->  out bf16 [B][N][128]
// One work-group = 4 waves = 128 queries of one (image, head); one wave = one 32-query tile.  Flash form over 32-key tiles on v_mfma_f32_32x32x16_bf16, with
// the swapped products of the fp32 kernel (kernels_misc.hip: full_attn_kernel):
//   S^T  = K Q^T     A = K rows, B = Q rows: 2 MFMAs.  The accumulator has the query on the lane and the 32 keys of the tile in the 16 registers of the
//                    two lane halves: row = (reg&3) + 8(reg>>2) + 4(lane>>5)
//   online softmax   over the lane's 16 registers + one cross-half shuffle, fp32
//   O^T += V^T P^T   A = V^T, B = the lane's own P registers packed to bf16 (no lane movement, no LDS): registers 8s .. 8s+7 are the fragment of k-step s,
//                    element j of lane half h being key 16s + 8(j>>2) + 4h + (j&3) — the V^T fragment is laid out in LDS in that same key order
// Rounding points: q, k, v as stored; the scale 32^-1/2 multiplies the fp32 scores; max / exponent / rescale in fp32; P rounded to bf16 (RNE) and the row sum
// adds the ROUNDED P, so the weights that multiply V sum to one; O / l in fp32, rounded once on the store.
// The K and V tiles (2 KB each) are staged in LDS once per work-group, double-buffered: the global loads of tile t + 1 are issued before the products of
// tile t and stored behind them — one barrier per tile.  No atomics, no workspace: deterministic and capturable.
#include "common.h"

namespace irsde {

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16_t;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

constexpr int kHeads = 4;
constexpr int kDh = 32;
constexpr int kHid = kHeads * kDh;  // 128
constexpr int kQkv = 3 * kHid;      // 384
// LDS row of a staged tile: 32 bf16 + 8 of padding = 80 bytes.  The 16-byte fragment reads of 16 consecutive rows then start 20 banks apart and
// cover the 64 banks once.
constexpr int kRow = 40;

__global__ __launch_bounds__(256) void full_attn16_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, const int N, const float scale) {
    __shared__ __attribute__((aligned(16))) bf16_t Ks[2][32 * kRow];   // [key][d]
    __shared__ __attribute__((aligned(16))) bf16_t Vt[2][32 * kRow];   // [d][key slot]: slot 16s + 8h + j holds key 16s + 8(j>>2) + 4h + (j&3)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int bh = blockIdx.y, b = bh >> 2, head = bh & 3;
    const int q0 = (blockIdx.x * 4 + wave) * 32;
    const bool live = q0 < N;   // wave-uniform; a wave without queries still stages its share of every tile and meets every barrier
    const bf16_t* base = qkv + (size_t)b * N * kQkv + head * kDh;
    const int q = q0 + l31;
    bf16x8 qf[2];   // B operand of S^T: Q[query l31][d = 16s + 8h + j]
    {
        const bf16_t* qp = base + (size_t)min(q, N - 1) * kQkv + 8 * h;
        qf[0] = *reinterpret_cast<const bf16x8*>(qp);
        qf[1] = *reinterpret_cast<const bf16x8*>(qp + 16);
    }
    // staging: waves 0, 1 carry the K tile, waves 2, 3 the V tile; one 16-byte piece (8 channels of one key) per thread
    const bool is_v = tid >= 128;
    const int skey = (tid & 127) >> 2, sc = tid & 3;
    const int vslot = 16 * (skey >> 4) + 8 * ((skey >> 2) & 1) + 4 * ((skey >> 3) & 1) + (skey & 3);
    auto gload = [&](int j0) {
        const int j = j0 + skey;
        bf16x8 v = *reinterpret_cast<const bf16x8*>(base + (size_t)min(j, N - 1) * kQkv + (is_v ? 2 * kHid : kHid) + 8 * sc);
        if (is_v && j >= N) {   // keys behind the end weigh 0: their V rows are zeros, their K rows any finite row
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = (bf16_t)0.f;
        }
        return v;
    };
    auto sstore = [&](int buf, bf16x8 v) {
        if (!is_v) {
            *reinterpret_cast<bf16x8*>(&Ks[buf][skey * kRow + 8 * sc]) = v;
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) Vt[buf][(8 * sc + i) * kRow + vslot] = v[i];
        }
    };
    float m = -INFINITY, l = 0.f;
    floatx16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
    const int ntiles = (N + 31) >> 5;
    sstore(0, gload(0));
    __syncthreads();
    for (int t = 0; t < ntiles; ++t) {
        const int buf = t & 1, j0 = t << 5;
        const bool more = t + 1 < ntiles;   // block-uniform
        bf16x8 nxt;
        if (more) nxt = gload(j0 + 32);
        if (live) {
            floatx16 st;
#pragma unroll
            for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const bf16x8 kf = *reinterpret_cast<const bf16x8*>(&Ks[buf][l31 * kRow + 16 * s + 8 * h]);   // K[key l31][d = 16s + 8h + j]
                st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[s], st, 0, 0, 0);
            }
            float tmax = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int jj = j0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                st[r] = jj < N ? st[r] * scale : -INFINITY;
                tmax = fmaxf(tmax, st[r]);
            }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
            const float mnew = fmaxf(m, tmax);   // finite: key j0 of every tile exists
            const float alpha = expf(m - mnew);
            bf16x8 pf[2];
            float psum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const bf16_t p = (bf16_t)expf(st[r] - mnew);   // RNE
                pf[r >> 3][r & 7] = p;
                psum += (float)p;
            }
            psum += __shfl_xor(psum, 32, 64);
            l = l * alpha + psum;
            m = mnew;
#pragma unroll
            for (int r = 0; r < 16; ++r) o[r] *= alpha;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const bf16x8 vf = *reinterpret_cast<const bf16x8*>(&Vt[buf][l31 * kRow + 16 * s + 8 * h]);   // V[key of slot 16s + 8h + j][d = l31]
                o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[s], o, 0, 0, 0);
            }
        }
        if (more) sstore(buf ^ 1, nxt);   // that buffer was last read before the previous barrier
        __syncthreads();
    }
    if (live && q < N) {
        const float il = 1.0f / l;
        bf16_t* op = out + ((size_t)b * N + q) * kHid + head * kDh;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {  // registers 4g .. 4g+3 are d = 8g + 4h + {0..3}
            bf16x4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = (bf16_t)(o[4 * g4 + i] * il);
            *reinterpret_cast<bf16x4*>(op + 8 * g4 + 4 * h) = v;
        }
    }
}

}  // namespace

void launch_full_attention16(const unsigned short* qkv, unsigned short* out, int B, int N, hipStream_t s) {
    if (B < 1 || N < 1 || B * kHeads > 65535) throw HipError("full_attention16: bad shape");
    if ((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(out)) & 15) throw HipError("full_attention16: tensors must be 16-byte aligned");
    const int qtiles = (N + 31) / 32;
    hipLaunchKernelGGL(full_attn16_kernel, dim3((qtiles + 3) / 4, B * kHeads), dim3(256), 0, s, reinterpret_cast<const bf16_t*>(qkv),
                       reinterpret_cast<bf16_t*>(out), N, 1.0f / sqrtf((float)kDh));
    IRSDE_HIP_CHECK(hipGetLastError());
}

}  // namespace irsde
