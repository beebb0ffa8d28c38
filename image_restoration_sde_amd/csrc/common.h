// Shared declarations for the IR-SDE gfx950 engine (internal; the public C ABI is include/irsde_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>
#include "split3_layout.h"

namespace irsde {

struct HipError : std::runtime_error {
    using std::runtime_error::runtime_error;
};
struct HipOutOfMemory : HipError {   // a device allocation failed: the plan cache evicts and retries (engine_plan.hip, get_plan)
    using HipError::HipError;
};

// Tuning knobs (A/B experiments logged under profiles/) are honoured only when IRSDE_TUNING=1 is set: a stray
// environment variable must not change the launch plan the parity tests validated.  Returns the integer value of
// `name`, or `dflt` when tuning is off or the variable is unset.
inline int tuning_env_int(const char* name, int dflt) {
    static const bool on = [] { const char* t = getenv("IRSDE_TUNING"); return t && atoi(t) == 1; }();
    if (!on) return dflt;
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}

#define IRSDE_HIP_CHECK(expr)                                                                  \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            throw ::irsde::HipError(std::string(#expr) + " failed: " + hipGetErrorString(_e) + \
                                    " (" __FILE__ ":" + std::to_string(__LINE__) + ")");       \
        }                                                                                      \
    } while (0)

// ---------------------------------------------------------------------------------------------
// Implicit-GEMM convolution, NHWC fp32, exact-fp32 MFMA (v_mfma_f32_32x32x2_f32).
//   out[m][n] = epilogue( sum_{ky,kx,c} in[(b, oy*stride-pad_y+ky, ox*stride-pad_x+kx), c] * w[n][ky][kx][c] )
// with m = (b*Ho + oy)*Wo + ox.  The input may be the channel-concatenation of two tensors
// (torch.cat([x, skip], 1) is never materialised) and may be read through a nearest x2 upsample
// (in_shift = 1: virtual pixel (y,x) reads physical (y>>1, x>>1)).
// Epilogue order: +bias[n] -> *(film_scale[n]+1)+film_shift[n] -> SiLU -> +res[m][n].
// ---------------------------------------------------------------------------------------------
struct ConvParams {
    const float* in0 = nullptr;
    const float* in1 = nullptr;  // second concat source or null
    int C0 = 0, C1 = 0;          // channels looped per source (multiples of 32)
    int pix0 = 0, pix1 = 0;      // floats between consecutive pixels of each source
    int Hin = 0, Win = 0;        // physical input height/width (both sources)
    int in_shift = 0;            // 1: fused nearest x2 upsample
    const float* w = nullptr;    // [Cout][KH*KW][C0+C1]
    const unsigned short* w_bf = nullptr;  // same layout rounded to bf16: selects the bf16-MFMA kernel (fp32 accumulate)
    int f16 = 0;                 // 1: w_bf / w_pair hold IEEE fp16 (IRSDE_FLAG_FP16 / _SPLIT_F16X2): v_mfma_f32_32x32x16_f16
    // split-operand arithmetic on fp32 storage (IRSDE_FLAG_SPLIT_BF16X2 / _F16X2; conv_igemm.hip PAIR kernels): the weights as two
    // pair-interleaved 16-bit pieces [Cout][KH*KW*(C0+C1) / 32][hi 32 | lo 32] (split_pairs_kernel); fp16: pieces of w * 2^k, pair_scale = 2^-k
    const unsigned short* w_pair = nullptr;
    float pair_scale = 1.f;
    int Cout = 0;
    int KH = 1, KW = 1, stride = 1, pad_y = 0, pad_x = 0;
    int B = 0, Ho = 0, Wo = 0;
    float* out = nullptr;
    int out_stride = 0;          // floats between consecutive output pixels (>= Cout)
    const float* bias = nullptr;
    const float* film = nullptr;  // row r: [scale(Cout) | shift(Cout)]
    int film_bstride = 0;         // floats between rows of different batch items (0: one shared row)
    int silu = 0;
    const float* res = nullptr;   // [M][res_stride]
    int res_stride = 0;
    // split-K (small-M layers): partial sums are written to `partial` [splits][M][Cout] and the
    // epilogue runs in conv_splitk_reduce.
    int splits = 1;
    float* partial = nullptr;
    const float* zeros = nullptr;  // >= 16 zero bytes: out-of-image taps are loaded from here (address select, no branch)
    // --- NAFNet (Refusion) fusions -------------------------------------------------------------------------
    const float* ch_scale = nullptr;  // [Cout]: v *= ch_scale[n] after the activation, before +res  (beta / gamma)
    const float* in_scale = nullptr;  // [B][C0]: input element (b, k) is multiplied by in_scale[b][k] while staged (SCA)
    int gate = 0;      // SimpleGate epilogue: weight rows are interleaved (2j <- j, 2j+1 <- j + Cout/2); writes the Cout/2
                       // products out[m][j] = v[2j] * v[2j+1]  (out_stride counts the gated width)
    const float* gate_film = nullptr;  // gate epilogue only: product j *= (gate_film[b][j] + 1), += gate_film[b][Cout/2 + j]
    int gate_film_bstride = 0;         // floats between the rows of different batch items (latent-bokeh lens FiLM)
    int shuffle = 0;   // PixelShuffle(2) epilogue: weight rows ordered n' = (dy*2+dx)*Cout/4 + co; writes (and adds res at)
                       // out[b][2y+dy][2x+dx][co]  (out/res tensors are [B][2Ho][2Wo][Cout/4])
    // batched launch (Winograd: 16 independent GEMMs): blockIdx.z = k offsets the three tensors (floats)
    int nz = 1;
    long long z_in = 0, z_w = 0, z_out = 0;
    int no_direct_epi = 0;  // tuning (irsde_bench_conv variant 7 / IRSDE_NO_DIRECT_EPI): LDS-transposed epilogue in the f32 BUFA kernels too
    // bf16 activation storage (IRSDE_FLAG_BF16_ACT, bf16-MFMA kernels only): in0/in1 resp. out/res point at bf16 tensors
    // (strides in elements); accumulation and the epilogue arithmetic stay fp32
    int in_bf16 = 0, out_bf16 = 0;
    // IEEE fp16 activation storage (IRSDE_FLAG_F16_ACT, fp16-MFMA implicit-GEMM kernels only): in0/in1 resp. out/res point at fp16 tensors (strides in
    // elements).  The two sides are independent: the NAFNet's intro reads the fp32 prepped input, its ending writes the fp32 eps_hat
    int in_f16 = 0, out_f16 = 0;
    // channel LayerNorm fused into the epilogue (LinearAttention.to_out = Conv2d + LayerNorm, module_util.py:158-161, then the
    // Residual add): v = (v - mean_n v) * rsqrt(var_n v + eps) * ln_g[n], applied after bias and before +res.  Needs the
    // whole output row in one tile: Cout == 64 or 128, no split-K.
    const float* ln_g = nullptr;
    float ln_eps = 1e-5f;
};

// Winograd F(m x m,3x3) transforms (wino.hip).  Tiles: T = B * TH * TW with TH = Ho/m, TW = Wo/m.
struct WinoParams {
    const float* in0 = nullptr;
    const float* in1 = nullptr;
    int C0 = 0, C1 = 0, Hin = 0, Win = 0, in_shift = 0;
    int B = 0, TH = 0, TW = 0, T = 0;
    int tile = 2;               // output tile edge m of F(m x m, 3x3): 2 or 4; components = (m+2)^2
    float* V = nullptr;         // [(m+2)^2][T][C0+C1]
    // split-operand mode (gemm_split.hip): V is written as `nplanes` 16-bit pieces instead, in the layout v_pairs / v_triples names
    unsigned short* Vs = nullptr;
    int nplanes = 0;
    int v_f16 = 0;              // pairs only: 1 = IEEE fp16 pieces of V * v_scale (v_scale a power of two), 0 = bf16 pieces of V
    float v_scale = 1.f;
    int v_pairs = 0;            // 1: two planes, pair-interleaved: element (k, t, c, p) at Vs + ((k * T + t) * (Ctot / 32) + c / 32) * 64 + p * 32 + c % 32
    int v_triples = 0;          // 1: three bf16 planes in the row-pair-interleaved layout of split3_layout.h: element (k, t, c, p) at
                                //    Vs + k * split3_comp_elems(T, Ctot) + split3_index(t, c, p, Ctot / 32)
    const float* M = nullptr;   // [(m+2)^2][T][Cout]
    int Cout = 0;
    float* out = nullptr;
    int out_stride = 0;
    const float* bias = nullptr;
    const float* film = nullptr;
    int film_bstride = 0;
    int silu = 0;
    const float* res = nullptr;
    int res_stride = 0;
};
void launch_wino_input(const WinoParams& p, hipStream_t s);
// Polyphase Winograd F(4x4,2x2) for the resampling convolutions (wino.hip): 25 products per 16 outputs and phase.
//   down (up = 0): Conv2d 4x4 stride 2 pad 1 = the sum over the four input pixel phases (p, q) of a 2x2 correlation with taps w[2a+p][2b+q]; the phases join
//                  Cin in the K walk: V [25][T][4 Cin] (K index = (2p+q) Cin + c), U [25][Cout][4 Cin], M [25][T][Cout]; tile = 4x4 output pixels
//   up   (up = 1): nearest x2 + Conv2d 3x3 pad 1 = four OUTPUT phases (py, px), each a 2x2 correlation over the low-resolution map with phase-summed taps:
//                  V [4][25][T][Cin], U [4][25][Cout][Cin], M [4][25][T][Cout] (z = (2py+px) 25 + component); tile = 4x4 low-resolution = 8x8 output pixels
// T = B * TH * TW, TH / TW = ceil(tiled extent / 4); ragged edges are masked.  Epilogue: + bias.
struct WinoPolyParams {
    int up = 0;
    const float* in = nullptr;  // [B][Hin][Win][C]
    int C = 0, Hin = 0, Win = 0;
    int B = 0, TH = 0, TW = 0, T = 0;
    float* V = nullptr;
    unsigned short* Vs = nullptr;   // != nullptr: V as three bf16 planes in the layout of split3_layout.h instead (component z, row t, K index as above)
    int thread_writer = 0;          // up + Vs: 1 = the per-thread writer (the whole-line writer's bit-identity twin: irsde_debug_conv 28, IRSDE_WINO_POLY_LINES=0)
    const float* M = nullptr;
    int Cout = 0, Ho = 0, Wo = 0;
    float* out = nullptr;       // [B][Ho][Wo][out_stride]
    int out_stride = 0;
    const float* bias = nullptr;
};
void launch_wino_poly_input(const WinoPolyParams& p, hipStream_t s);
void launch_wino_poly_output(const WinoPolyParams& p, hipStream_t s);
// host: U of the layouts above from the packed weights [Cout][KH][KW][Cin] (up = 0: 4x4, 25 * Cout * 4 Cin floats; up = 1: 3x3, 100 * Cout * Cin floats)
void wino_poly_transform_weights(const float* w_packed, int Cout, int Cin, float* U, int up);
// fp32-equivalent GEMMs on the bf16 MFMA pipe (gemm_split.hip): C_z[m][n] = sum_k A_z[m][k] B_z[n][k] with both operands given
// as 2 or 3 16-bit planes (hi / mid / lo pieces of the f32 value), f32 accumulate, z = 0 .. ncomp-1.
struct SplitGemmArgs {
    const unsigned short* a = nullptr;  // component z at a + z * pA, b + z * pB, in the launcher's interleaved layout
    const unsigned short* b = nullptr;
    float* out = nullptr;               // element (z, m, n) at out + z * pO + m * ldc + n
    long long plA = 0, plB = 0, pA = 0, pB = 0, pO = 0;   // (plA / plB / lda: read by no kernel; kept so that the kernels' argument block stays as it was)
    int M = 0, N = 0, K = 0, lda = 0, ldc = 0;
    float out_scale = 1.f;              // fp16 pairs: the power of two that undoes the operand scales (applied to the accumulators)
    int n_inner = 1;                    // set by the launcher: the component count
    int nblk_n = 0;                     // set by the launcher
};
void gemm_split_global_init();
// two planes in the pair-interleaved layout [row][k / 32][plane][32 k] (v3 kernel: LDS-DMA, 256 x 256 tiles); pA / pB = elements
// per component and plane (M * K resp. N * K)
// f16: IEEE binary16 pieces (hi + lo = 22+ significand bits: fp32-equivalent products) instead of bf16 (16 bits); a.out_scale undoes
// the power-of-two scales the operand writers applied to stay inside fp16's range
void launch_gemm_split_pairs(const SplitGemmArgs& a, int ncomp, hipStream_t s, int abl = 0, bool f16 = false);
void launch_split_pairs(const float* in, unsigned short* out, size_t rows, int K, hipStream_t s, bool f16 = false,
                        float scale = 1.0f);  // f32 [rows][K] -> pair-interleaved hi / lo (f16: of in * scale)
// three bf16 planes in the row-pair-interleaved layout of split3_layout.h (gemm_split3i_kernel: six products, LDS-DMA, 256 x 128 tiles): the default path of
// the exact-fp32 engine's deep component GEMMs.  pA / pB = unsigned shorts per component (split3_comp_elems).
// Split3Launch picks the instance: the defaults are what every plan runs.
struct Split3Launch {
    enum Abl { FULL = 0, NO_LOADS = 1, NO_MFMA = 3, NO_STORES = 4 };   // the measurement twins of the PROBES build: no global loads in the K loop / MFMAs / output stores
    enum Tri { RULE, ON, OFF };                                         // RULE: the tuning knob, else the default
    Abl abl = FULL;
    Tri walk = RULE;    // ON: the persistent launch (at most one block per CU, each walking its share of the items), OFF: one item per block (its bit-identity twin);
                        // RULE: IRSDE_SPLIT3_WALK (default on)
    Tri drain = RULE;   // ON: the walk with vmcnt(0) in front of every barrier of the K loop (the ring's twin), OFF: the ring; RULE: IRSDE_SPLIT3_DRAIN (default off)
};
void launch_gemm_split_triples(const SplitGemmArgs& a, int ncomp, hipStream_t s, const Split3Launch& o = {});
void set_force_split3_blocks(int n);   // irsde_debug_force_split3_blocks: caps the persistent launch's grid (>= 8); -1 = one block per CU
bool gemm_split_triples_fits(long long M, long long N, long long K, long long ldc);   // K % 32 == 0 and every component slice inside the 32-bit offset range
void launch_split_triples(const float* in, unsigned short* out, int ncomp, size_t rows, int K, hipStream_t s);   // f32 [ncomp][rows][K] -> that layout
// The plain 1x1 convolution on three bf16 pieces with the A operand split INSIDE the kernel (gemm_split3a_kernel; "a" = activations in f32):
//   out[m][n] = sum_k A[m][k] W[n][k] (+ bias[n]),   A = up to two f32 NHWC sources side by side (in0: C0 channels, pixel stride pix0; in1: C1, pix1),
// W as the triples launch_split_triples writes for [N][K = C0 + C1].  Bit-identical to split_triples_kernel on A followed by gemm_split3i_kernel.
struct Split3aArgs {
    const float* in0 = nullptr;
    const float* in1 = nullptr;   // second source or null (C1 = 0)
    int C0 = 0, C1 = 0;           // multiples of 32: a 32-k step lies in one source
    int pix0 = 0, pix1 = 0;       // floats between consecutive rows (pixels) of each source
    const unsigned short* w3 = nullptr;
    const float* bias = nullptr;  // [N] or null
    float* out = nullptr;         // element (m, n) at out + m * out_stride + n
    int M = 0, N = 0, out_stride = 0;
    int nblk_n = 0;               // set by the launcher
};
// every source and the weight triples inside the 32-bit offset range, C0 / C1 multiples of 32; why_not (optional) names the first reason
bool gemm_split3a_fits(const Split3aArgs& a, const char** why_not = nullptr);
int gemm_split3a_blocks(long long M, int N, int cus, bool walk = true);   // the launch's grid: pure (the cap of irsde_debug_force_split3_blocks comes on top)
constexpr size_t kSplit3aLds = (size_t)2 * (256 * 128 + 128 * 192);
void launch_gemm_split3a(const Split3aArgs& a, hipStream_t s, const Split3Launch& o = {});   // (o.walk / o.drain RULE = the production walk with the ring)
// Does a direct-path layer run on gemm_split3a_kernel?  A pure function of its arguments (it reads neither the environment nor a device).
//   p: the layer as Builder::conv() has it in front of push_conv (p.splits: what push_conv would choose);  exact_f32: the engine's arithmetic is the exact-fp32
//   one and the plan is not the naive one;  master: split3_mode();  knob: split3_1x1_mode() (0 never, 1 the measured rule, 2 wherever eligible);  cus: CU count
struct Split3x1Choice {
    bool adopt = false;
    const char* why_not = "";   // the first reason of a refusal
    int grid = 0, lds = 0;
};
Split3x1Choice split3_1x1_choose(const ConvParams& p, bool exact_f32, int master, int knob, int cus);
Split3aArgs split3_1x1_args(const ConvParams& p, const unsigned short* w3);   // the kernel's arguments of an adopted layer
void launch_split_planes(const float* in, unsigned short* out, size_t n, size_t plane, int nplanes, hipStream_t s, bool f16 = false,
                         float scale = 1.0f);  // f32 -> bf16 pieces (f16: two IEEE fp16 pieces of in * scale), plane-major
void launch_wino_output(const WinoParams& p, hipStream_t s);
void wino_transform_weights(const float* w_packed, int Cout, int Cin, float* U, int tile);  // host
// Fused Winograd F(4x4,3x3) convolution (wino_fused.hip): transforms and the 36 component GEMMs in one kernel.  `p` is the
// plain 3x3 s1 p1 convolution (as for launch_conv), Uf the weights from wino_fused_pack_weights.
bool wino_fused_eligible(const ConvParams& p);
void wino_fused_pack_weights(const float* U, int Cout, int Cin, float* Uf);  // host: U[36][Cout][Cin] -> fragment order
void launch_wino_fused(const ConvParams& p, const float* Uf, hipStream_t s, unsigned long long* dbg = nullptr, int dflags = 0);
int wino_fused_num_blocks(const ConvParams& p);
// 16 tiles x 64 couts per work item (Cout and Cin multiples of 64), one persistent block per CU; its own weight fragment order
bool wino_fused64_eligible(const ConvParams& p);
void wino_fused64_pack_weights(const float* U, int Cout, int Cin, float* Uf);
void launch_wino_fused64(const ConvParams& p, const float* Uf, hipStream_t s, int variant = 0);
void wino_fused64_set_debug(unsigned long long* buf);   // stamp buffer of launch variants 25 / 28 / 29 (irsde_bench_conv 435, 2001, 2002)
// the fp16-pair kernel (variant 4): V is split as V / 16, the weights as scale * U (scale a power of two), p.pair_scale undoes both
constexpr float kWinoFused64PairVScale = 0.0625f;
void launch_wino_fused64_split_weights(const float* Uf, unsigned short* out, size_t nfloats, float scale, hipStream_t s);
int wino_fused64_num_blocks(const ConvParams& p);
bool wino_fused64_xcd_nb(const ConvParams& p);   // the launch maps cout blocks to XCDs (layers whose input is small next to U x rounds)
void wino_fused_global_init();
int device_cu_count();   // compute units of the CURRENT device, cached per device ordinal (conv_igemm.hip)
// r06: 32 tiles x 64 couts per work item, every weight fragment feeds two tile groups (wino_fused_t.hip); weights = wino_fused64_pack_weights order
bool wino_fused64t_eligible(const ConvParams& p);
long long wino_fused64t_num_items(const ConvParams& p);
void launch_wino_fused64t(const ConvParams& p, const float* Uf, hipStream_t s, int variant = 0);
void wino_fused64t_set_debug(unsigned long long* buf);   // stamp buffer of launch variant 5
void wino_fused_t_global_init();
// fused NAFBlock chain (naf_chain.hip): consecutive 512-channel NAFBlocks on an 8 x 8 feature map, one work-group per image
void naf_chain_global_init();
void naf_chain_set_debug(unsigned long long* buf);   // stamp buffer of launch variant 11: [B][8 waves][16]
bool naf_chain_shape_ok(int H, int W, int c);
size_t naf_chain_weight_halves(int nblocks);   // fp16 fragment streams [8 waves][nblocks][448 fragments][512]
size_t naf_chain_vec_floats(int nblocks);      // fp32 per-channel vectors [nblocks][NV_TOTAL = 14848]
void launch_naf_chain(const float* x, float* out, const unsigned short* w, const float* vecs, int nblocks, int B, const float* film, int film_bstride,
                      int film_off, const float* cam, int cam_bstride, int cam_off, hipStream_t s, int variant = 0);
// r06: G = 2 / 4 work-groups per image (the groups trade operand slices through L2; see naf_chain.hip)
std::vector<int> naf_chain_split_order(int nblocks, int G);   // fragment permutation: split stream position -> one-group stream position
void naf_chain_build_split_weights(const unsigned short* w1, unsigned short* dst, int nblocks, int G, hipStream_t s);
size_t naf_chain_split_scratch_bytes(int B);
int naf_chain_split_groups(int B, int G);                     // work-groups that must be co-resident
void launch_naf_chain_split(const float* x, float* out, const unsigned short* wG, const float* vecs, int nblocks, int B, const float* film, int film_bstride,
                            int film_off, const float* cam, int cam_bstride, int cam_off, int G, void* scratch, hipStream_t s);
const unsigned* naf_chain_split_error_flag(const void* scratch, int B);
void naf_chain_split_reset(void* scratch, int B);
void naf_chain_set_sabotage(int on);   // PROBES build: one group per image never arrives (test of the spin limit)
void attention_global_init();

double conv_flops(const ConvParams& p);  // 2*M*Cout*K (algorithmic)
// Tuning overrides of ONE launch_conv call (the kernel-level hooks of engine_debug.hip; never part of a kernel's arguments).  The default is the production dispatch.
struct ConvTune {
    enum Tile { TILE_AUTO, TILE_128, TILE_256x128, TILE_256, TILE_128_ONE_PER_CU };
    enum Halo { HALO_AUTO, HALO_OFF, HALO_FORCE_512, HALO_FORCE_256 };
    enum ZLoop { ZLOOP_AUTO, ZLOOP_OFF, ZLOOP_ALL, ZLOOP_PAIRS, ZLOOP_FORCE_1X1 };
    enum Order { ORDER_AUTO, ORDER_N_FAST, ORDER_N_SLOW };
    bool rules_off = false;        // off: the IRSDE_SMALL_BN(_F32) narrowing, the vector-pipe 3-channel kernel, the automatic 256 x 256 tile of the f32 kernels
    Tile tile = TILE_AUTO;         // f32, Cout >= 128: 256x128 / 256 / one 128 x 128 block per CU (120 KB of LDS); 16-bit operands and PAIR: 256 / 128
    bool no_buffer_desc = false;   // f32: generic pointer staging instead of buffer descriptors
    bool no_direct_epi = false;    // f32: LDS-transposed instead of direct epilogue
    Halo halo = HALO_AUTO;         // 16-bit operands, eligible 3x3 layers: generic tiles / the 512-pixel x 128-channel / the 256-pixel halo kernel
    ZLoop zloop = ZLOOP_AUTO;      // tile-loop kernel: both forms off / its batch-loop form with all / 2 components per block / forced (2 row tiles) for 1x1 layers
    Order halo_order = ORDER_AUTO; // halo kernels, tile order inside an XCD's range: by rule / output-channel blocks fastest / slowest (where there are >= 2 of them)
};
// The tuning knobs the kernel choice reads (IRSDE_<FIELD NAME>, DESIGN.md "Tuning knobs"); the defaults are the production values.  conv_knobs_from_env
// reads the environment once per process.
struct ConvKnobs {
    int small_bn = 2, small_bn_f32 = 0;         // block slots per CU an under-filled grid narrows its column tiles for (0 = rule off): 16-bit operands / f32
    int pair_tile256 = 1, pair_inscale256 = 0;  // PAIR: the 256 x 256 tile at all / for the SCA-scaled layers too (that instance spills)
    int no_bufa = 0;                            // f32: generic pointer staging instead of buffer descriptors
    int zloop = -1, zloop_1x1 = -1;             // tile-loop kernel: 0 = off, n = fixed batch resp. row tiles per block, -1 = by shape
    int zloop_maxnk = 32, zloop_minblk = 1024, zloop_deep = 1, zloop_ragged64 = 2048;
};
const ConvKnobs& conv_knobs_from_env();
// What launch_conv_halo runs for one layer of the halo family (conv_halo.hip): conv_halo_choose is a pure function of its arguments.
struct HaloChoice {
    int pixels = 0;                    // pixels per block: 256 (conv3x3_halo_bf16_kernel, 16 x 16) or 512 (conv3x3_halo2_kernel, 16 x 32)
    int BN = 0;                        // output channels per block: 64 / 128
    int op = 0, act = 0;               // ConvChoice::Operand (2 bf16, 3 fp16) and ConvChoice::Storage (0 f32, 1 bf16) by number
    int tiles_x = 0, tiles_y = 0, nblk_n = 0;
    int n_slow = 0;                    // 1: the output-channel blocks run slowest inside an XCD's range
    unsigned grid = 0;
    int lds = 0;
    int instance = -1;                 // 0 .. 8, in the order conv_halo_global_init lists the kernels
};
constexpr int kHaloInstances = 9;
// What launch_conv runs for one layer: conv_choose is a pure function of its arguments (no device, no environment), conv_validate holds launch_conv's refusals.
struct ConvChoice {
    enum Family { PAIR, NARROW3, ZLOOP_BATCH, ZLOOP_1X1, HALO, IGEMM };
    enum Operand { OP_F32, OP_F32_BUF, OP_BF16, OP_F16 };   // f32 MFMA with generic pointers / buffer descriptors; the 16-bit MFMA (PAIR: the pieces' type)
    enum Storage { ACT_F32, ACT_BF16, ACT_F16 };            // what the kernel's staging reads
    Family family = IGEMM;
    int BM = 0, BN = 0;
    Operand op = OP_F32;
    Storage act = ACT_F32;
    bool inscale = false;
    int zbatch = 0, zrows = 0;         // tile-loop forms: components resp. row tiles per block
    unsigned gx = 0, gy = 1, gz = 1;   // HALO: conv_halo.hip chooses its own kernel and grid (gx == 0 here)
    HaloChoice halo;                   // HALO: what launch_conv_halo launched — filled by launch_conv, not by conv_choose (instance -1)
    int threads = 0, lds = 0;
    int row = -1;                      // index into the instance tables (implicit-GEMM / PAIR rows first, then the tile-loop rows); -1: the family has none, or no such instance
    std::string name() const;          // stable short name: igemm128x64, pair256x256, zloop64x128, zloop1x1_128x128, narrow3, halo
    long long blocks() const { return (long long)gx * gy * gz; }
};
int conv_base_bn(int Cout);   // column-tile width before any narrowing: 128 / 64 / 32
void conv_validate(const ConvParams& p);
ConvChoice conv_choose(const ConvParams& p, const ConvTune& t, const ConvKnobs& k, int cu_count);
int conv_instance_count();    // rows of the instance tables
// knobs: the tuning knobs of this one call (null: conv_knobs_from_env(), what every production caller runs on); chosen: receives the choice the launch made
void launch_conv(const ConvParams& p, hipStream_t s, const ConvTune& t = {}, const ConvKnobs* knobs = nullptr, ConvChoice* chosen = nullptr);
void conv_global_init();
// bf16 mode: 3x3 s1 p1 layers with an LDS-resident halo tile (conv_halo.hip)
void conv_halo_global_init();
bool conv_halo_eligible(const ConvParams& p);
// Kernel (256 / 512 pixels), BN, tile order, grid and LDS bytes of one eligible layer: no HIP call, no static, no environment.  t.halo forces a kernel
// (HALO_FORCE_512 where the layer has >= 128 output channels and fits its descriptors), t.halo_order a tile order; halo2 / nslow are the values of
// IRSDE_HALO2 (1: the 512-pixel kernel where its rule wants it, 0: never by rule) and IRSDE_HALO_NSLOW (-1: by rule, 0 / 1: the order for every layer).
// Throws for a layer the family does not take.
HaloChoice conv_halo_choose(const ConvParams& p, const ConvTune& t, int halo2, int nslow);
bool conv_halo2_wanted(const ConvParams& p);   // the production choice is the 512-pixel x 128-channel kernel (irsde_plan_describe names it)
HaloChoice launch_conv_halo(const ConvParams& p, hipStream_t s, const ConvTune& t = {});   // returns what it launched
void launch_fill_random(float* p, size_t n, unsigned seed, float scale, hipStream_t s);  // sets the dynamic-LDS attribute of every tile configuration (call before graph capture)
// SiLU for the epilogues of the f32 MFMA kernels: v_exp_f32 + v_rcp_f32 (1 ulp each) — 5 vector instructions instead of the
// ~25 of expf() + IEEE division.  On gfx950 the vector instructions of an f32-MFMA kernel are paid in matrix-pipe time
// (tools/probe/mfma_valu_*.hip); the epilogue SiLU was a third of the fused Winograd kernel's vector instructions.
// |result - v / (1 + exp(-v))| <= ~3e-7 |result| (the exponent product adds |v| 2^-24 relative to e^-v, which only matters
// where SiLU itself is ~0); e^-v = inf gives v * 0.
__device__ __forceinline__ float silu_hw(const float v) {
    return v * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(v * -1.44269504088896341f));
}

void launch_f32_to_bf16(const float* in, unsigned short* out, size_t n, hipStream_t s);  // round-to-nearest-even
void launch_f32_to_f16(const float* in, unsigned short* out, size_t n, hipStream_t s);   // IEEE binary16, round-to-nearest-even
void launch_bf16_to_f32(const unsigned short* in, float* out, size_t n, hipStream_t s);
void launch_f16_to_f32(const unsigned short* in, float* out, size_t n, hipStream_t s);
// naive direct convolution on VALU (one thread per output) — debug / cross-check path only
void launch_conv_naive(const ConvParams& p, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Memory-bound helpers (kernels_misc.hip)
// ---------------------------------------------------------------------------------------------
// Channel LayerNorm over C per pixel (gain only, eps inside rsqrt), optional residual add.
// bf16 = true: x / res / out are bf16 tensors behind the float* (IRSDE_FLAG_BF16_ACT); arithmetic stays fp32.
void launch_layernorm(const float* x, const float* g, const float* res, float* out, int64_t M, int C,
                      float eps, hipStream_t s, bool bf16 = false);
// NAFNet: y = LN(x) * g * (scale + 1) + shift with per-channel FiLM rows (row stride film_bstride per batch item, 0 = shared)
void launch_layernorm_film(const float* x, const float* g, const float* scale, const float* shift, int film_bstride,
                           int64_t pixels_per_image, float* out, int64_t M, int C, float eps, hipStream_t s,
                           bool f16 = false);   // f16: x and out are IEEE fp16 tensors behind the float* (IRSDE_FLAG_F16_ACT)
// NAFNet: depthwise 3x3 (pad 1, bias) over u [B][H][W][2c] fused with SimpleGate -> out [B][H][W][c], plus per-tile
// channel sums partial[b][tile][c] (deterministic two-stage global average pool).  w: [9][2c], bias: [2c].
int dwgate_tiles(int H, int W, int c);
// r06: NAFBlock norm + FiLM + 1x1 convolution (+ SimpleGate) in one launch, fp16 operand mode, c = 64 / 128 / 256 (kernels_misc.hip)
bool naf_lnconv_ok(int c, int Cout, long long M);
void launch_naf_pwconv(const float* x, const float* in_scale, int64_t pixels_per_image, const unsigned short* w16, const float* bias, const float* ch_scale,
                       const float* res, float* out, int64_t M, int c, int Cout, hipStream_t s, bool f16 = false);   // f16: x, res and out are fp16 tensors
void naf_lnconv_global_init();
void launch_naf_lnconv(const float* x, const float* g, const float* fscale, const float* fshift, int film_bstride, int64_t pixels_per_image,
                       const unsigned short* w16, const float* bias, float* out, int64_t M, int c, int Cout, int gate, const float* gate_film,
                       int gate_film_bstride, hipStream_t s, bool f16 = false);  // f16: x and out are fp16 tensors
// tiles of launch_dwconv_gate = rows of its `partial` buffer per image
void launch_dwconv_gate(const float* u, const float* w, const float* bias, float* out, float* partial, int B, int H, int W,
                        int c, hipStream_t s, bool f16 = false);   // f16: u and out are fp16 tensors; partial stays fp32, summed before the store rounding
// NAFNet SCA: s[b][o] = bias[o] + sum_k W[o][k] * mean_hw(gated)[b][k]
void launch_sca(const float* partial, int ntiles, const float* W, const float* bias, float* mean, float* s_out, int B,
                int c, int HW, hipStream_t s);  // mean: scratch [B][c]
// the pooled mean alone: mean[b][k] = sum_tiles partial[b][tile][k] / HW (launch_sca's first stage on large maps; the one-launch form forms the same bits in LDS)
void launch_sca_mean(const float* partial, int ntiles, float* mean, int B, int c, int HW, hipStream_t s);
// TLSC local pooling of CNAFNetLocal (tlsc_pool.hip): window means of the gated tensor [B][h][w][c] over k1 x k2 windows -> pooled
// [B][h - k1 + 1][w - k2 + 1][c] (rowsum: scratch [B][h][w - k2 + 1][c]); gated *= the replicate-padded scale map of the same compact shape
void tlsc_check_shape(int B, int h, int w, int c, int k1, int k2);   // throws HipError: c a positive multiple of 4, 1 <= k1 <= h, 1 <= k2 <= w
void launch_tlsc_pool(const float* gated, float* rowsum, float* pooled, int B, int h, int w, int c, int k1, int k2, hipStream_t s);
void launch_tlsc_scale(float* gated, const float* scale, int B, int h, int w, int c, int k1, int k2, hipStream_t s);
// out[r][j] = in[r][j] * in[r][j + h]  (SimpleGate on time-embedding rows)
void launch_row_gate(const float* in, float* out, int rows, int h, hipStream_t s);

struct AttnWorkspace {
    float* pmax = nullptr;   // [B][nch][128]
    float* pctx = nullptr;   // [B][4][nch][1024]
    float* psum = nullptr;   // [B][4][nch][32]
    float* ctx = nullptr;    // [B][4][32][32]
    int nch = 0;             // N-chunks per image
};
int attn_chunk_len(int N, int B);    // pixels per context chunk (a multiple of 8, at least one 128-pixel tile)
int attn_num_chunks(int N, int B);
// qkv: [B][N][384] (q | k | v, 4 heads x 32 each).  out: [B][N][128].
void launch_linear_attention(const float* qkv, float* out, int B, int N, const AttnWorkspace& ws, hipStream_t s,
                             bool bf16 = false);

// Fused forms of the same block (linear_attn.hip).  What the three projections run on; LayerNorm, softmax and the context products are fp32 in every mode.
enum class AttnMode : int {
    F32 = 0,       // the fp32 weights alone
    PairF16 = 1,   // fp16 hi + lo planes [2][rows][K] of w * 2^k, *_inv = 2^-k (IRSDE_FLAG_SPLIT_F16X2)
    Bf16 = 2,      // one unscaled bf16 plane (IRSDE_FLAG_BF16); act_bf16: xn / x / y are bf16 tensors (IRSDE_FLAG_BF16_ACT)
    Fp16 = 3,      // one unscaled IEEE fp16 plane (IRSDE_FLAG_FP16)
    Bf16x3 = 4,    // three unscaled bf16 planes in MFMA-fragment order (launch_split_frag3), six products: the exact-fp32 engine (IRSDE_SPLIT3_ATTN)
};
struct AttnProj {
    AttnMode mode = AttnMode::F32;
    bool act_bf16 = false;
    const unsigned short *kv = nullptr, *q = nullptr, *out = nullptr;   // planes of the [256][C] k | v rows, the [128][C] q rows, to_out.0.weight [C][128]
    float kv_inv = 1.f, q_inv = 1.f, out_inv = 1.f;
};
bool attn_fused_has_instance(int C, AttnMode mode, bool act_bf16);   // do both fused kernels exist for this shape and mode?
// The kernel-level hooks' view of the two instance tables (engine_debug.hip; host only, nothing is launched).  attn_require_instance: throws what the k / v
// (q_out: the q + out) launcher would throw for this shape and mode.  attn_choice: the rows a launch would take (-1: none), their dynamic LDS, the pixels per
// tile and the chunk geometry of attn_chunk_len / attn_num_chunks.
void attn_require_instance(bool q_out, int C, AttnMode mode, bool act_bf16);
struct AttnChoice {
    int kv_row = -1, kv_rows = 0, qo_row = -1, qo_rows = 0;
    size_t kv_lds = 0, qo_lds = 0;
    int kv_tile = 0, qo_tile = 0, chunk_len = 0, nch = 0;
};
AttnChoice attn_choice(int C, AttnMode mode, bool act_bf16, int N, int B);
// k, v, their softmax and the context from xn and wkv (the k | v rows of to_qkv.weight) without a k / v tensor in HBM.
// ln_g != nullptr: `xn` is the un-normalised block input and PreNorm's LayerNorm (* ln_g, eps) runs inside the kernel.
void launch_attention_kv_context(const float* xn, const float* wkv, int B, int N, int C, const AttnWorkspace& ws, hipStream_t s,
                                 const float* ln_g = nullptr, float ln_eps = 1e-5f, const AttnProj& proj = {});
// Fragment order of one plane of a [rows][K] matrix: [row / 32][k / 16][(k % 16) / 8][row % 32][k % 8] — lane (l31 = row % 32, h) of a wave finds its 8 values of
// (32-row tile, 16-k step) at 16-byte slot ((row tile * K / 16 + step) * 64 + 32 h + l31): one contiguous KB per wave load
__host__ __device__ inline size_t attn_frag3_index(size_t row, int k, int K) {
    return ((((row >> 5) * (size_t)(K >> 4) + (size_t)(k >> 4)) * 2 + (size_t)((k >> 3) & 1)) * 32 + (row & 31)) * 8 + (size_t)(k & 7);
}
void launch_split_frag3(const float* in, unsigned short* out, size_t rows, int K, hipStream_t s);   // out: [3][rows * K]
void launch_attention_q_out(const float* q, float* out, int B, int N, const AttnWorkspace& ws, hipStream_t s);
// C = 64 / 128 / 256: q projection, softmax over d, context product, to_out (+ bias), LayerNorm (* g2) and the residual in one
// kernel: y = LayerNorm(Wout . (ctx^T softmax(Wq . xn)) + bias) * g2 + x.  wq = rows 0..127 of to_qkv.weight ([128][C]),
// wout = to_out.0.weight ([C][128]); needs ws.ctx from launch_attention_kv_context.
void launch_attention_q_out_fused(const float* xn, const float* x, const float* wq, const float* wout, const float* bias,
                                  const float* g2, float* y, int B, int N, int C, float eps, const AttnWorkspace& ws, hipStream_t s,
                                  const float* ln_g = nullptr, const AttnProj& proj = {});

// Stereo-sr SCAM (scam.hip): x [2B][H][W][c] NHWC, views stacked [L_0..L_{B-1}, R_0..R_{B-1}]; H' = H / 4, W' = W / 4 (floor).
//   prologue  xs2 [2B][H'][W'][LN(xs) (norm_l / norm_r gain) | xs], xs = bicubic quarter-downsample of x
//   core      qv [2B][H'][W'][Q | V] -> F [2B][H'][W'][c]: F_r2l in the left images, F_l2r in the right ones
//   epilogue  out = x + (beta | gamma)[ch] * F[nearest]
void scam_check_shape(int H, int W, int c, bool any_width = false);   // throws HipError for maps the reference cannot run (H or W < 4) or the kernels do not cover
                                                                      // (any_width: the core is the streaming one, the strip limit W / 4 <= 512 does not apply)
void launch_scam_prologue(const float* x, const float* g_l, const float* g_r, float* xs2, int B, int H, int W, int c, hipStream_t s);
void launch_scam_core(const float* qv, float* F, int B, int H, int W, int c, hipStream_t s);
void launch_scam_epilogue(const float* x, const float* F, const float* beta, const float* gamma, float* out, int B, int H, int W, int c, hipStream_t s);
void scam_pack_proj(const float* w1, const float* b1, const float* w2, const float* b2, int c, std::vector<float>& w, std::vector<float>& bias);
// Full-resolution SCAM of the stereo-sr ConditionalUNet (scam.hip; DenoisingUNet_arch.py:18-56): no downsample, no upsample, H' = H, W' = W.
//   prologue  x2 [2B][H][W][LN(x) (norm_l / norm_r gain) | x]
//   core      qv [2B][H][W][Q | V] -> F [2B][H][W][c]
//   epilogue  x += (beta | gamma)[ch] * F, in place
constexpr int kScamFullMaxW = 1024;   // widest row: the 16 x W score strip (and nothing else of S) lives in LDS
constexpr int kScamFullMaxC = 2048;
void scam_full_check_shape(int H, int W, int c, bool any_width = false);   // throws HipError for shapes the kernels do not cover (any_width: as above, W <= 1024 dropped)
void launch_scam_full_prologue(const float* x, const float* g_l, const float* g_r, float* x2, int B, int H, int W, int c, hipStream_t s);
void launch_scam_full_core(const float* qv, float* F, int B, int H, int W, int c, hipStream_t s);
void launch_scam_full_epilogue(float* x, const float* F, const float* beta, const float* gamma, int B, int H, int W, int c, hipStream_t s);
// Streaming core of both SCAMs (scam_stream.hip, IRSDE_FLAG_SCAM_STREAM): the strip cores' contract on the H' x W' map of each view, any W', the other view's
// row walked in column blocks of block_w (a multiple of 16 up to kScamStreamMaxBlockW; 0 = that maximum) with an online softmax.  Throws HipError for c outside
// [32, 2048] / not a multiple of 32, B * H' > 65535 and a bad block_w.
constexpr int kScamMaxWs = 512;               // widest quarter-map row of scam_core_kernel
constexpr int kScamStreamMaxBlockW = 512;     // a 33 KB score tile
bool scam_stream_block_ok(int block_w);       // a multiple of 16 in [16, kScamStreamMaxBlockW]
void launch_scam_stream_core(const float* qv, float* F, int B, int Hs, int Ws, int c, int block_w, hipStream_t s);
// stereo network glue: 6-channel pair tensors <-> the 2B-view network batch
void launch_stereo_prep(const float* xt, const float* cond, float* x0, int B, int ic, int P, int H, int W, int Hp, int Wp, hipStream_t s);
void launch_stereo_pack_pred(const float* in, float* out, int B, int ic, int Hp, int Wp, int in_stride, int out_stride, hipStream_t s);
// the stereo UNet's forms: cat(xt_v, cond_v) with the reflect pad, and eps_hat = xt + cat(x_l, x_r) (xt: the pair state [B][2 ic][H][W])
void launch_stereo_unet_prep(const float* xt, const float* cond, float* x0, int B, int ic, int P, int H, int W, int Hp, int Wp, hipStream_t s);
void launch_stereo_unet_pack_pred(const float* in, const float* xt, float* out, int B, int ic, int H, int W, int Hp, int Wp, int in_stride, int out_stride,
                                  hipStream_t s);

// Full softmax attention over N tokens (denoising-sde bottleneck): qkv [B][N][384] -> out [B][N][128].
void launch_full_attention(const float* qkv, float* out, int B, int N, hipStream_t s);
// The same on bf16 tensors (IRSDE_FLAG_BF16_ACT; full_attn16.hip): qkv bf16 [B][N][384] -> out bf16 [B][N][128], both 16-byte aligned.  Flash form on the bf16
// MFMA: q, k, v as stored, fp32 scores / max / exponent / rescale, P rounded to bf16 for P.V, O / l rounded once on the store.
void launch_full_attention16(const unsigned short* qkv, unsigned short* out, int B, int N, hipStream_t s);

// xt, cond: NCHW [B][3][H][W] (cond may be null: unconditional variant, channels = xt only).  x0: [B][Hp+6][Wp+6][8] (+8 floats slack), zero border of 3,
// channels {xt-cond (3), cond (3), 0, 0}, reflect-padded right/bottom from (H,W) to (Hp,Wp).
void launch_prep_input(const float* xt, const float* cond, float* x0, int B, int in_nc, int H, int W, int Hp, int Wp,
                       hipStream_t s, int reflect = 1);

// FiLM / time-embedding path.
//   temb0[r][i] = sin/cos(t_r * freq[i])          (SinusoidalPosEmb)
//   generic row-linear: out[r][o] = act_out( sum_i act_in(in[r][i]) * W[o][i] + b[o] )
enum Act { ACT_NONE = 0, ACT_SILU = 1, ACT_GELU = 2 };
void launch_sinusoid(const float* tvals, const float* freqs, float* out, int rows, int half, hipStream_t s);
void launch_row_linear(const float* in, int in_stride, const float* W, const float* b, float* out, int out_stride,
                       int rows, int in_dim, int out_dim, int act_in, int act_out, hipStream_t s);

// Per-step device state (lets one captured hipGraph replay for every t).
struct StepState {
    int t;           // current step (T..1)
    int t_next;      // step the next step_begin will take
    int pad0, pad1;
    float coef[12];  // row t of the coefficient table (see include/irsde_hip.h)
};
// cur.t = cur.t_next--, copy film_table[t] -> film_cur and coef_table[t] -> state.coef
void launch_step_begin(StepState* st, const float* film_table, int film_row, float* film_cur,
                       const float* coef_table, hipStream_t s);
void launch_set_step(StepState* st, int t_next, hipStream_t s);

// Per-call sampler arguments kept in device memory so that a captured graph stays call-invariant.
struct SampleCtl {
    int mode;
    int pad;
    const float* noise;
    long long noise_tstride;
    unsigned long long seed;
    unsigned long long image_offset;
};
void launch_set_ctl(SampleCtl* ctl, int mode, const float* noise, long long noise_tstride, unsigned long long seed,
                    unsigned long long image_offset, hipStream_t s);

// eps_hat [B][Hp][Wp][stride] (NHWC, padded) -> out [B][C][H][W] (crop)
void launch_unpack_pred(const float* pred, float* out, int B, int C, int H, int W, int Hp, int Wp, int stride, hipStream_t s);
void launch_add(const float* a, const float* b, float* out, size_t n, hipStream_t s);  // n % 4 == 0
// NCHW -> NHWC with channel padding to Cp (zeros) and spatial padding to (Hp, Wp) (reflect or zero)
void launch_nchw_to_nhwc_pad(const float* in, float* out, int B, int C, int H, int W, int Hp, int Wp, int Cp, int reflect,
                             hipStream_t s);
// NHWC [B][H][W][C] -> NCHW (debug taps)
void launch_nhwc_to_nchw(const float* in, float* out, int B, int C, int H, int W, hipStream_t s, bool bf16 = false, bool f16 = false);   // bf16 / f16: `in` is a 16-bit tensor

// Reverse-step update x <- f(x, mu, eps_hat, z) on NCHW state; eps_hat addressed by strides.
struct UpdateParams {
    float* x;            // [B][C][H][W] in/out
    const float* mu;     // [B][C][H][W]
    const float* pred;   // eps_hat, element (b,c,y,x) at pred[b*sb + c*sc + y*sy + x*sx]
    int64_t sb, sc, sy, sx;
    const float* noise;  // injected noise base [T+1][B][C][H][W] or null (=> Philox)
    int64_t noise_tstride;
    const StepState* st;  // device step state, or null => use t_imm / coef_imm
    const SampleCtl* ctl; // device per-call arguments (override mode/noise/seed/image_offset) or null
    int t_imm;
    float coef_imm[12];
    int mode;            // IRSDE: 0 sde, 1 ode, 2 posterior; DenoisingSDE: 3 sde, 4 ode
    int B, C, H, W;
    uint64_t seed;
    uint64_t image_offset;  // global index of image 0 of this shard (RNG invariance to sharding)
    int batch0;          // r05 sub-batch plans: x / mu / pred hold images [batch0, batch0 + B) of the call's batch — the injected noise tensor and the
                         // Philox image index are addressed with the call-level index b + batch0
};
void launch_sde_update(const UpdateParams& p, hipStream_t s);
// fills out[B][C][H][W] with the Philox N(0,1) draw for step t (test hook for the RNG)
void launch_philox_normal(float* out, int B, int CHW, int t, uint64_t seed, uint64_t image_offset, hipStream_t s);

// Evaluation tail (eval_metrics.hip): per-image sums for PSNR / SSIM on RGB and Y.  sums_host: [B][4] =
// {squared-error sum RGB, SSIM-map sum RGB, squared-error sum Y, SSIM-map sum Y}.  Synchronises the stream.
void eval_metrics(const float* out, const float* gt, int B, int C, int H, int W, int crop, double* sums_host, hipStream_t s);
void tensor2img_u8(const float* in, unsigned char* out, int B, int C, int H, int W, hipStream_t s);

// LPIPS v0.1 / AlexNet in fp32 (lpips.hip): the feature tower (prologue, five convolutions on the f32 MFMA with bias + ReLU, two max-pools) and the distance.
struct LpipsLayer { int k, stride, pad, cin, cout; };   // AlexNet `features`; a 3x3 stride-2 max-pool (floor mode) sits in front of layers 2 and 3
constexpr LpipsLayer kLpipsLayers[5] = {{11, 4, 2, 3, 64}, {5, 1, 2, 64, 192}, {3, 1, 1, 192, 384}, {3, 1, 1, 384, 256}, {3, 1, 1, 256, 256}};
inline int lpips_cin_padded(int l) { return (kLpipsLayers[l].cin + 3) & ~3; }   // conv1 runs on 4 input channels (the 4th is zero)
struct LpipsWeights {
    const float* w[5];     // conv l + 1, K-major [KH * KW * Cin][Cout], k = (ky * KW + kx) * Cin + ci (conv1: Cin padded from 3 to 4 with zero rows)
    const float* bias[5];  // [Cout]
    const float* lin[5];   // the 1x1 lin layer of tap l + 1: [C]
};
struct LpipsGeom {
    int h[5], w[5];    // the five taps' maps
    int ph[2], pw[2];  // the pooled maps in front of conv2 / conv3
};
LpipsGeom lpips_geometry(int H, int W);   // throws below 31 x 31
int lpips_dist_blocks(int hw);            // partial sums per image of a tap with hw pixels
size_t lpips_workspace_floats(int N, int H, int W);
void lpips_features(const LpipsWeights& wt, const float* in0, const float* in1, int B, int H, int W, int normalize, float* ws, float* taps[5], hipStream_t s,
                    const std::function<void(const char*)>& mark);
void lpips_distances(const LpipsWeights& wt, float* const taps[5], int B, int H, int W, double* partial, hipStream_t s,
                     const std::function<void(const char*)>& mark);

// Degradation front ends (degrade.hip): bicubic upscale by an integer factor 1..8 (NCHW fp32 -> [B][C][H scale][W scale]) and the inpainting
// composite mask * x + (1 - mask) with uint8 masks [Bm][Hm][Wm][Cm] resized by nearest interpolation.  Stream-ordered, no synchronisation.
void upscale_bicubic(const float* in, float* out, int B, int C, int H, int W, int scale, hipStream_t s);
void mask_to(const float* x, const unsigned char* masks, int Bm, int Hm, int Wm, int Cm, float* out, int B, int C, int H, int W, hipStream_t s);
// imresize (codes/data/util.py:305-387): NCHW fp32 [B][C][H][W] -> [B][C][Ho][Wo] through per-axis device tables wH[Ho][KH] / sH[Ho] and
// wW[Wo][KW] / sW[Wo] (weights and the image coordinate of each output's first tap; out-of-image taps read the symmetric extension); H pass first.
void imresize(const float* in, float* out, int B, int C, int H, int W, int Ho, int Wo, const float* wH, const int* sH, int KH, const float* wW,
              const int* sW, int KW, hipStream_t s);

}  // namespace irsde
