// Streaming SCAM core (IRSDE_FLAG_SCAM_STREAM): the cross-view attention of scam.hip for rows of any width.
//
// scam_core_kernel / scam_full_core_kernel keep the whole 16 x W' strip of one direction's score matrix in LDS and take an exact two-pass softmax
// over it, which bounds W' (512 / 1024).  This core walks the other view's row in column blocks of block_w columns instead and carries the softmax
// in online (flash) form: per strip row a running maximum m and sum l, and P . V accumulators that stay in registers across the blocks and are
// rescaled by alpha = exp(m_old - m_new) whenever the maximum moves.  Same contract as the strip cores:
//   qv [2B][H'][W'][Q (c) | V (c)] fp32, views stacked [L.. | R..]  ->  F [2B][H'][W'][c]
//   grid (ceil(W' / 16) strips, B * H' rows, 2 directions), 256 threads; direction 0: rows of S = Q_l Q_r^T times V_r, direction 1: rows of S^T times V_l
//   v_mfma_f32_16x16x4_f32 with the lane / k-permutation conventions of scam_full_core_kernel; every statistic and product fp32
// No atomics, no waiting between work-groups, no scratch in HBM; LDS: P[16][block_w + 4] + alpha[16] + 1 / l [16] (33 KB at block_w = 512).
#include "common.h"

namespace irsde {

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kStreamNT = kScamStreamMaxBlockW / 64;   // column tiles of one block per wave
constexpr int kPairGroup = 4;                          // channel pairs of a wave per pass of P . V

// NP: 32-channel pairs per wave (c <= 128 NP); the 2 NP accumulators of a wave live in registers for the whole row.
template <int NP>
__global__ void __launch_bounds__(256) scam_stream_core_kernel(const float* __restrict__ qv, float* __restrict__ F, int B, int H, int W, int c,
                                                               int bw, float scale) {
    extern __shared__ float lds[];
    const int ld = bw + 4;
    float* P = lds;
    float* alpha = lds + 16 * ld;
    float* linv = alpha + 16;
    const int strip = blockIdx.x, row = blockIdx.y, dir = blockIdx.z;
    const int b = row / H, h = row % H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l16 = lane & 15, kk = lane >> 4;
    const size_t rowsz = (size_t)W * 2 * c;
    const int own_img = dir == 0 ? b : B + b, oth_img = dir == 0 ? B + b : b;
    const float* own = qv + ((size_t)own_img * H + h) * rowsz;   // strip rows: Q at [0, c)
    const float* oth = qv + ((size_t)oth_img * H + h) * rowsz;   // other view: Q at [0, c), V at [c, 2c)
    const float* vb = oth + c;
    const int i0 = strip * 16;
    const int npair = c / 32;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    const int ia = i0 + l16;
    const bool a_ok = ia < W;
    const float* arow = own + (size_t)(a_ok ? ia : 0) * 2 * c + 4 * kk;

    f32x4 o0[NP], o1[NP];   // P . V of channel pair wave + 4 p: channels 32 cp + l16 / + 16, rows 4 kk + r
#pragma unroll
    for (int p = 0; p < NP; ++p) o0[p] = o1[p] = zero;
    // running statistics of strip row sr, held (equal) by its 16 lanes
    const int sr = threadIdx.x >> 4, sq = threadIdx.x & 15;
    float m_run = 0.f, l_run = 0.f;

    for (int j0 = 0; j0 < W; j0 += bw) {
        const int nb = min(bw, W - j0);          // valid columns of this block
        const int ntile = (nb + 15) >> 4, nbt = ntile * 16;
        // 1. S block [16][nbt] = scale * Q_own[i0 .. i0 + 15] . Q_oth[j0 ..]^T: k on the outside, the wave's tiles t = wave + 4 u in accumulators.  Lane
        //    (l16, kk) of k-block kb holds k = kb + 4 kk + s in MFMA step s for both operands (a k permutation shared by A and B leaves the sum unchanged).
        {
            f32x4 acc[kStreamNT];
#pragma unroll
            for (int u = 0; u < kStreamNT; ++u) acc[u] = zero;
            for (int k = 0; k < c; k += 32) {
                const f32x4 a0 = a_ok ? *reinterpret_cast<const f32x4*>(arow + k) : zero;
                const f32x4 a1 = a_ok ? *reinterpret_cast<const f32x4*>(arow + k + 16) : zero;
#pragma unroll
                for (int u = 0; u < kStreamNT; ++u) {
                    const int t = wave + 4 * u;
                    if (t < ntile) {   // (wave-uniform)
                        const int jb = j0 + t * 16 + l16;
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
            for (int u = 0; u < kStreamNT; ++u) {
                const int t = wave + 4 * u;
                if (t < ntile) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) P[(4 * kk + r) * ld + t * 16 + l16] = acc[u][r] * scale;
                }
            }
        }
        __syncthreads();
        // 2. online softmax of the 16 rows: block maximum over the nb valid columns, m_new = max(m, m_blk), alpha = exp(m - m_new) (0 in the first block:
        //    exp(-inf - -inf) is never evaluated), P = exp(S - m_new) with 0 in the padding columns, l = l alpha + sum P
        {
            float* pr = P + sr * ld;
            float mb = -INFINITY;
            for (int j = sq; j < nb; j += 16) mb = fmaxf(mb, pr[j]);
            for (int o = 8; o > 0; o >>= 1) mb = fmaxf(mb, __shfl_xor(mb, o, 16));
            const bool first = j0 == 0;
            const float m_new = first ? mb : fmaxf(m_run, mb);
            const float al = first ? 0.f : expf(m_run - m_new);
            float s = 0.f;
            for (int j = sq; j < nbt; j += 16) {
                const float e = j < nb ? expf(pr[j] - m_new) : 0.f;
                pr[j] = e;
                s += e;
            }
            for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 16);
            l_run = l_run * al + s;
            m_run = m_new;
            if (sq == 0) {
                alpha[sr] = al;
                linv[sr] = 1.0f / l_run;   // (l >= 1: the row maximum contributes exp(0)); read after the last block
            }
        }
        __syncthreads();
        // 3. acc = alpha[row] acc + P_blk . V_blk: lane (l16, kk) of j-block jb holds j = jb + 4 kk + s in step s (A from LDS as one float4, B as coalesced
        //    64-byte rows of V); one A read serves the kPairGroup channel pairs of a pass
        {
            f32x4 al;
#pragma unroll
            for (int r = 0; r < 4; ++r) al[r] = alpha[4 * kk + r];
#pragma unroll
            for (int p = 0; p < NP; ++p) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    o0[p][r] *= al[r];
                    o1[p][r] *= al[r];
                }
            }
#pragma unroll
            for (int pg = 0; pg < NP; pg += kPairGroup) {   // kPairGroup channel pairs per pass over the block: bounds the V loads in flight
                if (wave + 4 * pg >= npair) break;          // (wave-uniform)
#pragma unroll 1
                for (int jb = 0; jb < nbt; jb += 16) {
                    const f32x4 a = *reinterpret_cast<const f32x4*>(P + l16 * ld + jb + 4 * kk);
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const int j = j0 + jb + 4 * kk + s;
                        const bool j_ok = j < W;
                        const float* vr = vb + (size_t)(j_ok ? j : 0) * 2 * c + l16;
#pragma unroll
                        for (int p = pg; p < pg + kPairGroup && p < NP; ++p) {
                            const int cp = wave + 4 * p;
                            if (cp < npair) {   // (wave-uniform)
                                const float v0 = j_ok ? vr[cp * 32] : 0.f, v1 = j_ok ? vr[cp * 32 + 16] : 0.f;
                                o0[p] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], v0, o0[p], 0, 0, 0);
                                o1[p] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], v1, o1[p], 0, 0, 0);
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();   // P and alpha are rewritten by the next block
    }
    // F = acc / l
    float* fo = F + ((size_t)own_img * H + h) * (size_t)W * c;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int cp = wave + 4 * p;
        if (cp < npair) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int il = 4 * kk + r, i = i0 + il;
                if (i < W) {
                    fo[(size_t)i * c + cp * 32 + l16] = o0[p][r] * linv[il];
                    fo[(size_t)i * c + cp * 32 + 16 + l16] = o1[p][r] * linv[il];
                }
            }
        }
    }
}

template <int NP>
void launch_np(const float* qv, float* F, int B, int H, int W, int c, int bw, hipStream_t s) {
    const size_t lds = (size_t)(16 * (bw + 4) + 32) * sizeof(float);   // <= 33.2 KB: inside the default limit
    const dim3 grid((unsigned)((W + 15) / 16), (unsigned)(B * H), 2);
    hipLaunchKernelGGL(scam_stream_core_kernel<NP>, grid, dim3(256), lds, s, qv, F, B, H, W, c, bw, 1.0f / sqrtf((float)c));
}

}  // namespace

bool scam_stream_block_ok(int block_w) { return block_w >= 16 && block_w <= kScamStreamMaxBlockW && block_w % 16 == 0; }

void launch_scam_stream_core(const float* qv, float* F, int B, int H, int W, int c, int block_w, hipStream_t s) {
    if (B < 1 || H < 1 || W < 1) throw HipError("SCAM (streaming): empty feature map");
    if (c % 32 || c < 32 || c > kScamFullMaxC) throw HipError("SCAM (streaming): channel count must be a multiple of 32 in [32, 2048]");
    if ((long long)B * H > 65535) throw HipError("SCAM (streaming): more than 65535 image rows in one launch");
    if (block_w != 0 && !scam_stream_block_ok(block_w)) throw HipError("SCAM (streaming): block_w must be 0 (the default) or a multiple of 16 in [16, 512]");
    const int Wt = (W + 15) & ~15;
    const int bw = std::min(block_w ? block_w : kScamStreamMaxBlockW, Wt);   // (a block wider than the row is one block)
    if (c <= 128) launch_np<1>(qv, F, B, H, W, c, bw, s);
    else if (c <= 256) launch_np<2>(qv, F, B, H, W, c, bw, s);
    else if (c <= 512) launch_np<4>(qv, F, B, H, W, c, bw, s);
    else if (c <= 1024) launch_np<8>(qv, F, B, H, W, c, bw, s);
    else launch_np<16>(qv, F, B, H, W, c, bw, s);
    IRSDE_HIP_CHECK(hipGetLastError());
}

}  // namespace irsde
