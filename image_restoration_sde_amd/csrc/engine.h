// libirsde_hip.so — engine internals shared by engine_weights.hip / engine_plan.hip / engine_api.hip / engine_debug.hip.
//
// Host-side structure (all C++; PyTorch never appears here):
//   Engine      weights in kernel layout, FiLM/time table, coefficient table, plans
//   Plan        per (B,H,W): static activation arena + the launch list of ONE network evaluation
//               (ConditionalUNet.forward, DenoisingUNet_arch.py:85-134) built once, replayed T times
//   sample()    the reverse loop (sde_utils.py:252-299): [step_begin, prep, net, update] per t, either
//               eager or as one captured hipGraph replayed T times; the step index lives in device
//               memory (StepState) so the graph is t-invariant.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/irsde_hip.h"
#include "common.h"

namespace irsde {

// Winograd only where the transforms' extra HBM traffic is small next to the GEMM: F(2x2) moves 4x the input and
// 4x the output through HBM and pays from 256 channels, F(4x4) 2.25x and pays from 128 — from 64 (+1.6 %) since the
// component GEMMs run on the batch-loop kernel (measured, profiles/).
// IRSDE_WINO2_MINC / IRSDE_WINO4_MINC override the thresholds (tuning experiments, only with IRSDE_TUNING=1).
// The fused Winograd kernel (wino_fused.hip) streams a layer's whole U slice per block: it pays where the feature map is
// large (many tiles) and the channel counts are moderate; beyond these limits the three-launch path keeps the layer.
constexpr int kWinoFusedMaxCin = 256, kWinoFusedMaxCout = 256;  // measured crossover (profiles/r02_wino_fused_sweep.txt): Cin 384+ is faster on the three-launch path
inline long long wino_fused_min_tiles() { return tuning_env_int("IRSDE_WINO_FUSED_MINT", 4096); }
// r03: the 64-cout fused kernel (16 tiles x 64 couts per block) takes the layers whose channel counts are multiples of 64;
// IRSDE_WINO_FUSED64=0 keeps them on the 32-cout kernel, IRSDE_WINO_FUSED64_MAXCIN / _MAXCOUT move its crossover (tuning only)
inline bool wino_fused64_enabled() { return tuning_env_int("IRSDE_WINO_FUSED64", 1) != 0; }
inline bool wino_fused64_pair_enabled() { return tuning_env_int("IRSDE_WINO_FUSED64_PAIR", 1) != 0; }   // fp32_split_f16: the kernel's fp16-pair twin
inline int wino_fused64_max_cin() { return tuning_env_int("IRSDE_WINO_FUSED64_MAXCIN", 512); }
inline int wino_fused64_max_cout() { return tuning_env_int("IRSDE_WINO_FUSED64_MAXCOUT", 512); }
inline long long wino_fused64_min_tiles() { return tuning_env_int("IRSDE_WINO_FUSED64_MINT", 1024); }
// r06: the two-tile-group kernel (wino_fused_t.hip) on the layers it measured faster on: 0 never, 1 by the rule of Plan::push_wino_fused, 2 wherever eligible
inline int wino_fused64t_mode() { return tuning_env_int("IRSDE_WINO_FUSED64T", 1); }
// r06: NAFBlock norm + 1x1 convolution as one launch on the small-channel levels of the fp16 operand mode (1; 0 = LayerNorm kernel + convolution kernel)
inline bool naf_lnconv_enabled() { return tuning_env_int("IRSDE_NAF_LNCONV", 1) != 0; }
// r06: work-groups per image of the NAFBlock chain kernel: 0 = as many (4, 2) as fit the compute units next to the call's other sub-batches, 1 = the one-group kernel, 2 / 4 forced (if they fit)
inline int naf_chain_split_mode() { return tuning_env_int("IRSDE_NAF_CHAIN_SPLIT", 0); }

// polyphase F(4x4,2x2) for the resampling convolutions of the exact-fp32 plans (wino.hip): 0 never, 1 by the rule of Builder::push_wino_poly, 2 wherever eligible
// (irsde_debug_force_wino_poly overrides the knob for engines created afterwards)
int wino_poly_mode();
void set_force_wino_poly(int mode);   // irsde_debug_force_wino_poly
// the rule's side that is known at weight-load time: every 4x4 stride-2 layer; nearest-x2 + 3x3 layers from 512 input channels (below that V and M, which the
// fused F(4x4,3x3) kernel keeps out of HBM, cost what the saved products gain: 256 -> 128 at 16 x 128^2 measured 1.45 against 1.47 ms, profiles/wino_poly.md)
constexpr int kWinoPolyUpMinCin = 512;
inline bool wino_poly_wants_weights(int mode, bool up, int Cin) { return mode >= 2 || (mode == 1 && (!up || Cin >= kWinoPolyUpMinCin)); }

// The exact-fp32 engine's deep component GEMMs on three bf16 pieces per operand and six products (gemm_split3i_kernel, gemm_split.hip): 0 never, 1 by the rule
// of Builder::split3_adopts, 2 wherever eligible (irsde_debug_force_split3 overrides the knob for engines created afterwards); IRSDE_FLAG_NO_SPLIT3 = never
int split3_mode();
void set_force_split3(int mode);   // irsde_debug_force_split3
// the rule's side that is known at weight-load time (profiles/split3.md, profiles/split3_walk.md): F(4x4,3x3) layers beyond the fused kernels' reach (Cin > 512),
// those with Cin = 512 and at least 512 output channels (mode 2: every layer), every polyphase layer
constexpr int kSplit3WinoMinCin = 512;
inline int split3_wino_min_cin() { return tuning_env_int("IRSDE_SPLIT3_MINCIN", kSplit3WinoMinCin); }   // (513: the Cin = 512 layers stay where they were)
inline bool split3_wino_wants_weights(int mode, int Cin, int Cout) { return mode >= 2 || Cin > 512 || (Cin >= split3_wino_min_cin() && Cout >= 512); }
// a layer the fused F(4x4,3x3) kernels would take leaves them for the three-launch path on triples from this many tiles on (IRSDE_SPLIT3_FUSED_MINT)
inline long long split3_fused_min_tiles() { return tuning_env_int("IRSDE_SPLIT3_FUSED_MINT", 4096); }
// every mode whose arithmetic is not the exact-fp32 engine's: the three-piece operands are never built there
constexpr int kSplit3NotExactF32 = IRSDE_FLAG_NO_WINOGRAD | IRSDE_FLAG_NAIVE_CONV | IRSDE_FLAG_BF16 | IRSDE_FLAG_BF16_ACT | IRSDE_FLAG_FP16 | IRSDE_FLAG_F16_ACT |
                                   IRSDE_FLAG_SPLIT_BF16X2 | IRSDE_FLAG_SPLIT_F16X2 | IRSDE_FLAG_NO_SPLIT3;
inline bool split3_wants_weights(int flags) { return !(flags & kSplit3NotExactF32) && split3_mode() > 0; }
// The same engine's fused LinearAttention blocks (C = 64 / 128 / 256) with their k / v, q and to_out projections on three bf16 pieces (linear_attn.hip, AttnMode::Bf16x3): 0 never,
// 1 by the rule of Builder::split3_attn_adopts, 2 wherever a kernel instance exists (irsde_debug_force_split3_attn overrides the knob for plans built afterwards).
// Off with the GEMMs' master switch (IRSDE_SPLIT3 = 0, IRSDE_FLAG_NO_SPLIT3); the master's mode 2 does not force it.
int split3_attn_mode();
void set_force_split3_attn(int mode);   // irsde_debug_force_split3_attn
// The same engine's plain 1x1 convolutions (bias-only epilogue: the res_conv of the up path, to_qkv of the unfused attention blocks) on three bf16 pieces with the
// activations split inside the GEMM (gemm_split3a_kernel): IRSDE_SPLIT3_1X1 = 0 never, 1 by the rule of split3_1x1_choose, 2 wherever eligible
// (irsde_debug_force_split3_1x1 overrides the knob for plans built afterwards).  Off with the master switch, which does not force it, as for the attention mode.
int split3_1x1_mode();
void set_force_split3_1x1(int mode);   // irsde_debug_force_split3_1x1

inline int wino_min_c(int tile) {
    return tuning_env_int(tile == 4 ? "IRSDE_WINO4_MINC" : "IRSDE_WINO2_MINC", tile == 4 ? 64 : 256);
}

// Selects the engine's device for the scope of one C-ABI call and restores the caller's current device afterwards
// (a multi-GPU host process — and PyTorch inside it — must not see its current device change under its feet).
struct DeviceScope {
    int prev = -1;
    explicit DeviceScope(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) IRSDE_HIP_CHECK(hipSetDevice(dev));
        else prev = -1;
    }
    ~DeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};

struct HostTensor {
    std::vector<int64_t> shape;
    std::vector<float> data;
    bool loaded = false;
};

struct ConvW {
    float* w = nullptr;  // device [Cout][KH*KW][Cin]
    float* bias = nullptr;
    int Cout = 0, Cin = 0, KH = 1, KW = 1;
    float* wino_u2 = nullptr;  // device [16][Cout][Cin] = G g G^T of F(2x2,3x3)  (3x3 layers with Cin,Cout >= 256)
    float* wino_u4 = nullptr;  // device [36][Cout][Cin]              F(4x4,3x3)  (3x3 layers with Cin,Cout >= 128)
    float* wino_uf = nullptr;  // the same F(4x4,3x3) weights in the fused kernel's fragment order (wino_fused.hip)
    float* wino_uf64 = nullptr;  // ... in the 64-cout fused kernel's fragment order (Cout, Cin multiples of 64)
    unsigned short* wino_uf64p = nullptr;   // IRSDE_FLAG_SPLIT_F16X2: wino_uf64 as fp16 hi / lo halves (wf64_split_weights_kernel), scaled by wino_uf64p_scale
    float wino_uf64p_scale = 1.f;
    unsigned short* wino_up = nullptr;  // IRSDE_FLAG_SPLIT_BF16X2 / _F16X2: the F(4x4,3x3) weights as hi / lo pairs, [36][Cout][Cin / 32][2][32]
    float wino_up_scale = 1.f;          // fp16 pairs: the power of two U was multiplied by (max |U| * scale <= 512)
    unsigned short* wino_u4t = nullptr;    // exact fp32, Cin > 512 (or = 512 with Cout >= 512): wino_u4 as three bf16 pieces, [36] x split3_layout.h of [Cout][Cin] (gemm_split3i_kernel's B operand)
    unsigned short* wino_polyt = nullptr;  // exact fp32: wino_poly as three bf16 pieces, [25 | 100] x split3_layout.h of [Cout][4 Cin | Cin]
    float* wino_poly = nullptr;  // polyphase F(4x4,2x2) weights (exact fp32 mode): 4x4 stride-2 layers [25][Cout][4 Cin], nearest-x2 + 3x3 layers [100][Cout][Cin]
};
struct ResW {
    ConvW b1, b2, res;
    bool has_res = false;
    float* mlp_w = nullptr;  // [2*Cout][time_dim]
    float* mlp_b = nullptr;
    int film_off = 0;
    int Cout = 0;
};
// SCAM(c): the fusion after every NAFBlock of the stereo-sr NAFNet (IRSDE_FLAG_NAF_STEREO; stereo-sr DenoisingNAFNet_arch.py:15-60, 131, on the quarter-resolution
// xs) and of the stereo-sr ConditionalUNet (IRSDE_FLAG_UNET_STEREO; stereo-sr DenoisingUNet_arch.py:18-35, at full resolution)
struct ScamW {
    int c = 0;
    float *gl = nullptr, *gr = nullptr;   // norm_l.g / norm_r.g
    ConvW l, r;                           // [[proj1, 0], [0, proj2]] per view: [LN(x) | x] (2c) -> [Q | V] (2c), bias [b1 | b2]
    float *beta = nullptr, *gamma = nullptr;
};
struct AttnW {
    float* g1 = nullptr;
    ConvW qkv, out;
    float* g2 = nullptr;
    int C = 0;
};

// NAFBlock weights (DenoisingNAFNet_arch.py:15-49) in kernel layout
struct NafBlockW {
    int c = 0;
    float *g1 = nullptr, *g2 = nullptr;          // norm1.g / norm2.g
    ConvW conv1, conv3, conv4, conv5;            // 1x1: c->2c, c->c, c->2c (rows interleaved for the gate), c->c
    float *dw_w = nullptr, *dw_b = nullptr;      // conv2 depthwise 3x3: [9][2c], [2c]
    float *sca_w = nullptr, *sca_b = nullptr;    // sca.1: [c][c], [c]
    float *beta = nullptr, *gamma = nullptr;
    float *mlp_w = nullptr, *mlp_b = nullptr;    // mlp.1: Linear(time_dim/2, 4c)
    int film_off = 0;                            // [shift_att | scale_att | shift_ffn | scale_ffn]
    float *cam_w = nullptr, *cam_b = nullptr;    // latent-bokeh: cam_mlp.1: Linear(time_dim/2, 2c)
    int cam_off = 0;                             // [cam_scale | cam_shift] inside a row of the lens table
    ScamW fusion;                                // stereo-sr (IRSDE_FLAG_NAF_STEREO): SCAM(c) after the block
};

// a run of consecutive 512-channel NAFBlocks packed for naf_chain_kernel (fp16 mode): fragment streams + fp32 vectors
struct NafChainW {
    unsigned short* w = nullptr;
    float* vecs = nullptr;
    int nblocks = 0, film_off = 0, cam_off = 0;
    unsigned short* wsplit[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // [G]: the fragment streams of the G-groups-per-image kernel, built on first use
};

// the reference-layout tensors of one such block (HOST pointers): what pack_naf_chain_host packs
struct NafChainHostW {
    const float *norm1_g, *conv1_w, *conv1_b, *conv2_w, *conv2_b, *sca_w, *sca_b, *conv3_w, *conv3_b, *beta, *norm2_g, *conv4_w, *conv4_b, *conv5_w, *conv5_b, *gamma;
};

enum OpKind { OP_CONV = 0, OP_LN = 1, OP_ATTN = 2, OP_OTHER = 3, OP_WINO = 4, OP_NKINDS = 5 };

struct Op {
    std::function<void(hipStream_t)> fn;
    OpKind kind;
    double flops = 0, bytes = 0;  // algorithmic (direct-convolution) work attributed to this launch group
    double exec_flops = 0;        // multiply-adds actually issued to the MFMA pipe (differs for Winograd)
    std::string desc;
};

// Winograd F(2x2,3x3) launch triple derived from the direct-form parameters of a 3x3 stride-1 pad-1 convolution
struct WinoPlan {
    WinoParams in, out;
    ConvParams gemm;
};
inline WinoPlan make_wino(const ConvParams& d, const float* U, float* V, float* Mb, int tile) {
    WinoPlan w;
    const int Ctot = d.C0 + d.C1;
    const int TH = d.Ho / tile, TW = d.Wo / tile, T = d.B * TH * TW;
    const int ncomp = (tile + 2) * (tile + 2);
    w.in.tile = tile;
    w.in.in0 = d.in0; w.in.in1 = d.in1; w.in.C0 = d.C0; w.in.C1 = d.C1; w.in.Hin = d.Hin; w.in.Win = d.Win;
    w.in.in_shift = d.in_shift; w.in.B = d.B; w.in.TH = TH; w.in.TW = TW; w.in.T = T; w.in.V = V;
    w.out = w.in;
    w.out.M = Mb; w.out.Cout = d.Cout; w.out.out = d.out; w.out.out_stride = d.out_stride; w.out.bias = d.bias;
    w.out.film = d.film; w.out.film_bstride = d.film_bstride; w.out.silu = d.silu; w.out.res = d.res;
    w.out.res_stride = d.res_stride;
    ConvParams& g = w.gemm;
    g.in0 = V; g.C0 = Ctot; g.pix0 = Ctot; g.Hin = 1; g.Win = T; g.w = U; g.Cout = d.Cout;
    g.KH = g.KW = 1; g.stride = 1; g.pad_y = g.pad_x = 0; g.B = 1; g.Ho = 1; g.Wo = T;
    g.out = Mb; g.out_stride = d.Cout; g.zeros = d.zeros;
    g.nz = ncomp; g.z_in = (long long)T * Ctot; g.z_w = (long long)d.Cout * Ctot; g.z_out = (long long)T * d.Cout;
    return w;
}
// Polyphase F(4x4,2x2) launch triple (wino.hip) of a 4x4 stride-2 pad-1 convolution (down) or a 3x3 pad-1 convolution behind the nearest x2 upsample (up)
inline bool wino_poly_down_shape(const ConvParams& d) {
    return d.KH == 4 && d.KW == 4 && d.stride == 2 && d.pad_y == 1 && d.pad_x == 1 && !d.in_shift && d.Hin >= 2 && d.Win >= 2;
}
inline bool wino_poly_up_shape(const ConvParams& d) { return d.KH == 3 && d.KW == 3 && d.stride == 1 && d.pad_y == 1 && d.pad_x == 1 && d.in_shift == 1; }
// single fp32 source, bias-only epilogue
inline bool wino_poly_eligible(const ConvParams& d) {
    return (wino_poly_down_shape(d) || wino_poly_up_shape(d)) && !d.in1 && !d.C1 && d.C0 % 32 == 0 && d.pix0 == d.C0 && d.Cout % 4 == 0 && d.out_stride % 4 == 0 &&
           !d.film && !d.silu && !d.res && !d.ln_g && !d.ch_scale && !d.in_scale && !d.gate && !d.shuffle && !d.in_bf16 && !d.out_bf16 && !d.in_f16 && !d.out_f16;
}
struct WinoPolyPlan {
    WinoPolyParams in, out;
    ConvParams gemm;
    int ncomp = 0;      // component GEMMs: 25 (down) / 100 (up)
    long long T = 0;
    int K = 0;          // 4 Cin (down) / Cin (up)
};
inline WinoPolyPlan make_wino_poly(const ConvParams& d, const float* U, float* V, float* Mb) {
    WinoPolyPlan w;
    const int up = d.in_shift ? 1 : 0;
    WinoPolyParams& q = w.in;
    q.up = up; q.in = d.in0; q.C = d.C0; q.Hin = d.Hin; q.Win = d.Win; q.B = d.B;
    q.Ho = d.Ho; q.Wo = d.Wo;
    q.TH = ((up ? d.Hin : d.Ho) + 3) / 4; q.TW = ((up ? d.Win : d.Wo) + 3) / 4; q.T = d.B * q.TH * q.TW;
    q.V = V; q.M = Mb; q.Cout = d.Cout; q.out = d.out; q.out_stride = d.out_stride; q.bias = d.bias;
    w.out = q;
    w.ncomp = up ? 100 : 25; w.T = q.T; w.K = up ? d.C0 : 4 * d.C0;
    ConvParams& g = w.gemm;
    g.in0 = V; g.C0 = w.K; g.pix0 = w.K; g.Hin = 1; g.Win = q.T; g.w = U; g.Cout = d.Cout;
    g.KH = g.KW = 1; g.stride = 1; g.pad_y = g.pad_x = 0; g.B = 1; g.Ho = 1; g.Wo = q.T;
    g.out = Mb; g.out_stride = d.Cout; g.zeros = d.zeros;
    g.nz = w.ncomp; g.z_in = (long long)q.T * w.K; g.z_w = (long long)d.Cout * w.K; g.z_out = (long long)q.T * d.Cout;
    return w;
}
// Split-operand variants (gemm_split.hip): V and the weights as `nplanes` 16-bit pieces in the GEMM kernel's interleaved layout, the component GEMMs on the
// 16-bit MFMA pipe, M and the output transform unchanged (f32)
struct WinoSplitPlan {
    WinoParams in, out;
    SplitGemmArgs gemm;
    int nplanes = 0;
    bool f16 = false;
};
// IRSDE_FLAG_SPLIT_BF16X2: pair-interleaved operands for launch_gemm_split_pairs (Vs: 36 * T * Ctot * 2 elements)
constexpr float kSplitF16VScale = 1.0f / 16.0f;   // fp16 pairs: V is written as V / 16 (finite up to |V| = 1e6)
inline WinoSplitPlan make_wino_pairs(const ConvParams& d, const unsigned short* Up, unsigned short* Vs, float* Mb, bool f16 = false,
                                     float u_scale = 1.f) {
    const WinoPlan w = make_wino(d, nullptr, nullptr, Mb, 4);
    WinoSplitPlan sp;
    sp.in = w.in; sp.out = w.out; sp.nplanes = 2;
    const int Ctot = d.C0 + d.C1;
    const long long T = w.in.T;
    sp.in.Vs = Vs; sp.in.nplanes = 2; sp.in.v_pairs = 1;
    sp.in.v_f16 = f16 ? 1 : 0; sp.in.v_scale = f16 ? kSplitF16VScale : 1.f;
    SplitGemmArgs& g = sp.gemm;
    g.out_scale = f16 ? 1.0f / (kSplitF16VScale * u_scale) : 1.f;
    sp.f16 = f16;
    g.a = Vs; g.b = Up; g.out = Mb;
    g.pA = T * Ctot; g.pB = (long long)d.Cout * Ctot; g.pO = T * d.Cout;
    g.M = (int)T; g.N = d.Cout; g.K = Ctot; g.lda = Ctot; g.ldc = d.Cout;
    return sp;
}
// exact fp32 on three bf16 pieces (gemm_split3i_kernel): Vs holds 36 components of split3_comp_elems(T, Ctot) unsigned shorts, Ut the weights' triples
inline WinoSplitPlan make_wino_triples(const ConvParams& d, const unsigned short* Ut, unsigned short* Vs, float* Mb) {
    const WinoPlan w = make_wino(d, nullptr, nullptr, Mb, 4);
    WinoSplitPlan sp;
    sp.in = w.in; sp.out = w.out; sp.nplanes = 3;
    const int Ctot = d.C0 + d.C1;
    const long long T = w.in.T;
    sp.in.Vs = Vs; sp.in.nplanes = 3; sp.in.v_triples = 1;
    SplitGemmArgs& g = sp.gemm;
    g.a = Vs; g.b = Ut; g.out = Mb;
    g.pA = (long long)split3_comp_elems((size_t)T, (size_t)Ctot); g.pB = (long long)split3_comp_elems((size_t)d.Cout, (size_t)Ctot); g.pO = T * d.Cout;
    g.M = (int)T; g.N = d.Cout; g.K = Ctot; g.lda = Ctot; g.ldc = d.Cout;
    return sp;
}
// the polyphase triple on three-piece operands: wp from make_wino_poly (V unused), Vs / Ut as above with K = wp.K
inline SplitGemmArgs make_wino_poly_triples(WinoPolyPlan& wp, int Cout, const unsigned short* Ut, unsigned short* Vs, float* Mb) {
    wp.in.Vs = Vs; wp.in.V = nullptr;
    SplitGemmArgs g;
    g.a = Vs; g.b = Ut; g.out = Mb;
    g.pA = (long long)split3_comp_elems((size_t)wp.T, (size_t)wp.K); g.pB = (long long)split3_comp_elems((size_t)Cout, (size_t)wp.K); g.pO = wp.T * Cout;
    g.M = (int)wp.T; g.N = Cout; g.K = wp.K; g.lda = wp.K; g.ldc = Cout;
    return g;
}
// split mode: three-launch Winograd layers with at least this many input channels run the pair GEMM (below it the fused
// f32 kernel is faster: profiles/r03_split_gemm_bench.txt); IRSDE_SPLIT_MINC moves the crossover (tuning only)
inline int split_min_cin() { return tuning_env_int("IRSDE_SPLIT_MINC", 256); }
// split mode: direct (implicit-GEMM) layers with K = KH * KW * Cin of at least this and >= 64 output channels run the PAIR kernel
// (conv_igemm.hip); below it the layer is HBM-bound and the native f32 kernel is as fast.  IRSDE_SPLIT_DIRECT_MINK (tuning only)
inline int split_direct_min_k() { return tuning_env_int("IRSDE_SPLIT_DIRECT_MINK", 128); }   // measured crossover: profiles/r03_pair_conv_sweep.txt
inline bool wino_shape_ok(const ConvParams& d, int tile) {
    return d.KH == 3 && d.KW == 3 && d.stride == 1 && d.pad_y == 1 && d.pad_x == 1 && d.Ho % tile == 0 && d.Wo % tile == 0 &&
           (d.C0 + d.C1) % 32 == 0 && d.Cout % 4 == 0 && d.out_stride % 4 == 0 && (!d.res || d.res_stride % 4 == 0);
}

// The power of two that brings max |host[i]| into (256, 512] (1 for all-zero input): the exact pre-scale of fp16 hi / lo operand pairs, undone by the
// kernel that consumes them
inline float pow2_scale_into_512(const float* host, size_t n) {
    float mx = 0.f;
    for (size_t i = 0; i < n; ++i) mx = std::max(mx, std::fabs(host[i]));
    return mx > 0.f ? std::exp2(std::floor(std::log2(512.0f / mx))) : 1.f;
}

struct Tensor {
    float* p = nullptr;  // bf16 == true: really a bf16 tensor (IRSDE_FLAG_BF16_ACT); f16 == true: an IEEE fp16 tensor (IRSDE_FLAG_F16_ACT)
    int B = 0, H = 0, W = 0, C = 0;
    bool bf16 = false, f16 = false;   // storage kind: at most one is set
    bool half() const { return bf16 || f16; }
    size_t numel() const { return (size_t)B * H * W * C; }
};

struct PoolBlock {
    float* p;
    size_t n;
    bool free;
};

struct Plan {
    int B = 0, H = 0, W = 0, Hp = 0, Wp = 0;
    bool per_sample_film = false;
    StepState* own_step = nullptr;   // sub-batch plans (slot >= 1) carry their own step counter / coefficient row and FiLM row: their step graphs replay
    float* own_film = nullptr;       // on their own stream with no per-step dependency on the other parts (both live in the plan's arena)
    int slot = 0, b0 = 0;     // r05 sub-batch plans: slot >= 1 = part `slot - 1` of a split batch, holding images [b0, b0 + B) of the call (own arena, own state buffers;
                              // per-image tables — lens FiLM rows, per-sample time rows, noise / Philox index — are addressed from b0)
    std::vector<PoolBlock> pool;
    std::vector<Op> net_ops;  // prep + network (one evaluation)
    float* xin = nullptr;     // [B][in_nc][H][W]  state x / xt
    float* cin = nullptr;     // [B][in_nc][H][W]  mu / cond
    float* x0 = nullptr;      // prepped NHWC input
    float* pred = nullptr;    // [B][Hp][Wp][pred_stride]
    int pred_stride = 4;      // roundup(out_nc, 4)
    std::map<std::string, Tensor> taps;
    hipGraphExec_t graph_exec = nullptr;
    hipGraph_t graph = nullptr;
    double conv_flops = 0, conv_bytes = 0, conv_exec_flops = 0;
    uint64_t last_use = 0;
    std::vector<std::pair<void*, int>> chain_scratch;   // (scratch, images) of the split chain launches, for the reset after an error
    std::vector<const unsigned*> chain_err;   // error flags of the split chain launches (naf_chain.hip): non-zero = the groups of an image were not co-resident

    ~Plan() {
        if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
        if (graph) (void)hipGraphDestroy(graph);
        for (auto& b : pool) (void)hipFree(b.p);
    }
    float* alloc(size_t n, bool reuse) {
        if (reuse) {
            int best = -1;
            for (int i = 0; i < (int)pool.size(); ++i)
                if (pool[i].free && pool[i].n >= n && (best < 0 || pool[i].n < pool[best].n)) best = i;
            if (best >= 0 && pool[best].n <= n + n / 2 + 1024) {
                pool[best].free = false;
                return pool[best].p;
            }
        }
        float* p = nullptr;
        const hipError_t err = hipMalloc(&p, std::max<size_t>(n, 64) * sizeof(float));
        if (err == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            throw HipOutOfMemory("plan arena: hipMalloc of " + std::to_string(std::max<size_t>(n, 64) * sizeof(float)) + " bytes failed (out of memory)");
        }
        IRSDE_HIP_CHECK(err);
        pool.push_back({p, n, false});
        return p;
    }
    void release(float* p) {
        for (auto& b : pool)
            if (b.p == p) {
                b.free = true;
                return;
            }
    }
};

// One direction (encode or decode) of the latent UNet at a fixed (B,H,W): a Plan whose ops run on NHWC buffers, plus
// the NHWC tensors that are read from / written to the caller's NCHW tensors around it.
struct LatentPlan {
    bool decode = false;
    std::unique_ptr<Plan> plan;
    Tensor image;                // encode: padded NHWC input image; decode: final_conv output [B][Hp][Wp][4]
    Tensor latent;               // NHWC latent (channels padded to 32)
    std::vector<Tensor> hidden;  // NHWC skips in the reference's list order h[0..2*depth]
    std::vector<int> hidden_c;   // logical channel counts
    bool resident = false;       // encode plan: the skips of the last encode are in place (decode plan: it SHARES the encode plan's skip tensors)
};

}  // namespace irsde

using namespace irsde;  // internal header: included only by the four engine_*.hip translation units

struct irsde_engine {
    irsde_config cfg{};
    int time_dim = 0;
    std::vector<std::string> names;  // weight inventory, reference state_dict order-independent
    std::map<std::string, HostTensor> host;
    bool finalized = false;
    std::vector<float*> dev_allocs;

    // packed weights
    ConvW init_conv, final_conv;
    float *tm_w1 = nullptr, *tm_b1 = nullptr, *tm_w3 = nullptr, *tm_b3 = nullptr, *freqs = nullptr;
    std::vector<ResW> down_res;   // 2 per level
    std::vector<AttnW> down_attn;
    std::vector<ConvW> down_conv;
    ResW mid1, mid2;
    AttnW mid_attn;
    std::vector<ScamW> down_scam, up_scam;   // IRSDE_FLAG_UNET_STEREO: downs.i.3 / ups.j.3
    ScamW mid_scam;                          // mid_fusion
    std::vector<ResW> up_res;
    std::vector<AttnW> up_attn;
    std::vector<ConvW> up_conv;
    ResW final_res;
    std::vector<ResW*> all_res;
    int film_row = 0;

    // ConditionalNAFNet (arch == 1)
    int arch = 0;
    int naf_ic = 0;   // the network's img_channel (cfg.in_nc is the sampler state's channel count: 2 naf_ic for IRSDE_FLAG_NAF_STEREO / _UNET_STEREO)
    std::vector<int> naf_enc_nums, naf_dec_nums;
    int naf_mid_num = 0;
    std::vector<std::vector<NafBlockW>> naf_enc, naf_dec;
    std::vector<NafBlockW> naf_mid;
    std::vector<ConvW> naf_downs, naf_ups;
    ConvW naf_intro, naf_ending;
    std::vector<NafBlockW*> naf_all;
    std::vector<NafChainW> naf_chain_enc, naf_chain_dec;   // per level (nblocks == 0: none)
    NafChainW naf_chain_mid;
    // latent-bokeh variant (IRSDE_FLAG_NAF_LENS): lens-information FiLM, one row per image of the batch
    float *cm_w1 = nullptr, *cm_b1 = nullptr, *cm_w3 = nullptr, *cm_b3 = nullptr;  // cam_mlp.0 / cam_mlp.2
    int cam_row = 0;            // sum over blocks of 2c
    float* cam_cur = nullptr;   // [cam_rows][cam_row]
    int cam_rows = 0;           // capacity (images)
    int cam_set = 0;            // images covered by the last irsde_set_lens_info

    // CNAFNetLocal (irsde_nafnet_set_local_pool): every NAFBlock's global average pool becomes a windowed mean (TLSC, local_arch.py:25-72) where the
    // window frozen at the training size is smaller than the block's map; 0 = the plain ConditionalNAFNet
    int tlsc_base_h = 0, tlsc_base_w = 0, tlsc_train_h = 0, tlsc_train_w = 0;

    // latent UNet (arch == 2): codes/config/latent-dehazing/models/modules/UNet_arch.py
    int lat_in = 0, lat_out = 0, lat_ch = 0, lat_embed = 0;
    std::vector<int> lat_mult;
    ConvW lat_init, lat_latent, lat_post, lat_final;
    std::vector<ResW> lat_enc_res, lat_dec_res;  // 2 per level (decoder in module order: deepest first)
    AttnW lat_enc_attn, lat_dec_attn;            // deepest level only
    std::vector<ConvW> lat_down, lat_up;
    std::vector<std::unique_ptr<LatentPlan>> lat_plans;

    // LPIPS v0.1 / AlexNet (arch == 3, irsde_create_lpips): no score network, no schedule, no plans; csrc/lpips.hip
    LpipsWeights lpips{};
    float* lpips_ws = nullptr;        // the tower's workspace, kept between calls and grown on demand
    size_t lpips_ws_floats = 0;
    double* lpips_partial = nullptr;  // the distance kernel's per-block partial sums
    size_t lpips_partial_n = 0;

    // schedule / FiLM tables
    int T = 0;
    float* coef_table = nullptr;  // [(T+1)][12]
    float* film_table = nullptr;  // [(T+1)][film_row]
    float* film_cur = nullptr;    // [max_rows][film_row]
    int film_cur_rows = 0;
    StepState* step = nullptr;
    SampleCtl* ctl = nullptr;

    float* zeros = nullptr;        // zero page: the branch-free source of out-of-image conv taps
    hipStream_t stream = nullptr;  // engine stream (graph capture needs a non-default stream)
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    // r05: concurrent sub-batches of a NAFNet sampler call (engine_api.hip: irsde_sample): part i > 0 runs all its steps on sub_stream[i - 1], forked once
    // behind the call's inputs (ev_fork) and joined once in front of its outputs (ev_join[i - 1])
    static constexpr int kMaxSub = 4;
    hipStream_t sub_stream[kMaxSub - 1] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[kMaxSub - 1] = {nullptr, nullptr, nullptr};
    std::vector<std::unique_ptr<Plan>> plans;
    uint64_t use_counter = 0;
    double profile[12] = {0};
    std::vector<double> op_ms;          // per launch group of the last profiled plan (summed over steps)
    std::vector<std::string> op_desc;
    int op_steps = 0;
    int plan_parts = 1;   // concurrent sub-batch plans the sampler call being prepared runs (set by irsde_sample around get_plan: the split chain's CU budget)
    int op_split = 1;   // concurrent sub-batches the sampler would run the profiled batch as (the event-instrumented pass times the un-split plan)
    std::vector<hipEvent_t> ev_pool;
    std::mutex mu;

    float* dmalloc(size_t n) {
        float* p = nullptr;
        IRSDE_HIP_CHECK(hipMalloc(&p, std::max<size_t>(n, 16) * sizeof(float)));
        dev_allocs.push_back(p);
        return p;
    }
    // bf16 / fp16 (RNE) copy of a packed fp32 weight tensor, made once per tensor (IRSDE_FLAG_BF16 / IRSDE_FLAG_FP16)
    std::map<const float*, unsigned short*> bf16_copies;
    const unsigned short* bf16_copy(const float* w, size_t n) {
        auto it = bf16_copies.find(w);
        if (it != bf16_copies.end()) return it->second;
        unsigned short* d = nullptr;
        IRSDE_HIP_CHECK(hipMalloc(&d, n * sizeof(unsigned short)));
        if (cfg.flags & IRSDE_FLAG_FP16) launch_f32_to_f16(w, d, n, stream);  // IEEE fp16 operands (RNE)
        else launch_f32_to_bf16(w, d, n, stream);
        IRSDE_HIP_CHECK(hipStreamSynchronize(stream));
        bf16_copies[w] = d;
        return d;
    }
    // hi / lo operand planes of a packed fp32 weight tensor for the PAIR convolution kernels (IRSDE_FLAG_SPLIT_BF16X2 / _F16X2), made
    // once per tensor.  fp16 pieces: the tensor is scaled by the power of two that brings max |w| into (256, 512]; `scale` returns
    // its inverse (what the kernel multiplies the accumulators by).
    struct PairCopy { unsigned short* p; float inv_scale; };
    std::map<const float*, PairCopy> pair_copies;
    PairCopy pair_copy(const float* w, size_t n) {
        return make_pair_copy(pair_copies, w, n, [&](unsigned short* d, bool f16, float sc) { launch_split_planes(w, d, n, n, 2, stream, f16, sc); });
    }
    // three unscaled bf16 planes [3][rows * K] of a packed fp32 [rows][K] weight matrix (hi, mid, lo: all 24 significand bits; bf16 has fp32's exponent range, so no
    // scale), made once per tensor and layout.  TRIPLES_FRAG3: MFMA-fragment order (attn_frag3_index), the fused attention kernels' three-piece projections;
    // TRIPLES_ROWPAIR: the row-pair-interleaved blocks of split3_layout.h, the B operand of gemm_split3a_kernel (the plain 1x1 convolutions)
    enum TripleLayout { TRIPLES_FRAG3 = 0, TRIPLES_ROWPAIR = 1 };
    std::map<std::tuple<const float*, int, size_t>, unsigned short*> triple_copies;   // (a q projection is the first 128 rows of its to_qkv tensor: the rows are part of the key)
    const unsigned short* triple_copy(const float* w, size_t rows, int K, TripleLayout layout = TRIPLES_FRAG3) {
        const auto key = std::make_tuple(w, (int)layout, rows);
        auto it = triple_copies.find(key);
        if (it != triple_copies.end()) return it->second;
        const size_t elems = layout == TRIPLES_ROWPAIR ? split3_comp_elems(rows, (size_t)K) : 3 * rows * (size_t)K;
        unsigned short* d = nullptr;
        IRSDE_HIP_CHECK(hipMalloc(&d, elems * sizeof(unsigned short)));
        dev_allocs.push_back(reinterpret_cast<float*>(d));
        if (layout == TRIPLES_ROWPAIR) launch_split_triples(w, d, 1, rows, K, stream);
        else launch_split_frag3(w, d, rows, K, stream);
        IRSDE_HIP_CHECK(hipStreamSynchronize(stream));
        triple_copies[key] = d;
        return d;
    }
    // The PAIR kernels of conv_igemm.hip read their weights pair-interleaved: [rows][K / 32][hi 32 | lo 32] (split_pairs_kernel), one
    // 128-byte line per 32-k block, fetched global -> LDS by global_load_lds.  K must be a multiple of 32.
    std::map<const float*, PairCopy> pair_copies_il;
    PairCopy pair_copy_il(const float* w, size_t rows, int K) {
        return make_pair_copy(pair_copies_il, w, rows * (size_t)K, [&](unsigned short* d, bool f16, float sc) { launch_split_pairs(w, d, rows, K, stream, f16, sc); });
    }
    // the two layouts' common part: cache lookup, scale, allocation, registration; split(d, f16, scale) launches the layout's kernel
    template <class Split>
    PairCopy make_pair_copy(std::map<const float*, PairCopy>& cache, const float* w, size_t n, Split split) {
        auto it = cache.find(w);
        if (it != cache.end()) return it->second;
        const bool f16 = (cfg.flags & IRSDE_FLAG_SPLIT_F16X2) != 0;
        float sc = 1.f;
        if (f16) {
            std::vector<float> h(n);
            IRSDE_HIP_CHECK(hipMemcpy(h.data(), w, n * sizeof(float), hipMemcpyDeviceToHost));
            sc = pow2_scale_into_512(h.data(), n);
        }
        unsigned short* d = nullptr;
        IRSDE_HIP_CHECK(hipMalloc(&d, 2 * n * sizeof(unsigned short)));
        dev_allocs.push_back(reinterpret_cast<float*>(d));
        split(d, f16, sc);
        IRSDE_HIP_CHECK(hipStreamSynchronize(stream));
        const PairCopy pc{d, 1.0f / sc};
        cache[w] = pc;
        return pc;
    }
    float* upload(const std::vector<float>& v) {
        float* p = dmalloc(v.size());
        IRSDE_HIP_CHECK(hipMemcpy(p, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
        return p;
    }
};

namespace irsde {

inline bool naf_lens(const irsde_engine* e) { return (e->cfg.flags & IRSDE_FLAG_NAF_LENS) != 0; }
inline bool naf_stereo(const irsde_engine* e) { return e->arch == 1 && (e->cfg.flags & IRSDE_FLAG_NAF_STEREO) != 0; }
inline bool unet_stereo(const irsde_engine* e) { return e->arch == 0 && (e->cfg.flags & IRSDE_FLAG_UNET_STEREO) != 0; }
inline bool stereo_engine(const irsde_engine* e) { return naf_stereo(e) || unet_stereo(e); }   // pair state, the network on the 2B views
// The networks without a condition input (denoising-sde): forward(x, time), DenoisingSDE sampler modes 3 / 4, cond / mu may be NULL
inline bool uncond_engine(const irsde_engine* e) {
    return (e->arch == 0 && (e->cfg.flags & IRSDE_FLAG_UNCOND_FULLATTN) != 0) || (e->arch == 1 && (e->cfg.flags & IRSDE_FLAG_NAF_UNCOND) != 0);
}
inline bool lpips_engine(const irsde_engine* e) { return e->arch == 3; }
inline int rup32(int c) { return (c + 31) & ~31; }
// CNAFNetLocal: the pool window (K0, K1) of the NAFBlocks at `level` (encoder i and decoder n_enc - 1 - i: level i; middle: n_enc) — what the reference's
// conversion forward on rand(train_size) freezes as kernel_size (local_arch.py:26-32): map size there x base_size / train_size.  false: no local pooling
inline bool tlsc_window(const irsde_engine* e, int level, int* K0, int* K1) {
    if (e->tlsc_train_h <= 0) return false;
    const int P = 1 << e->cfg.depth;
    const int Hp = (e->tlsc_train_h + P - 1) / P * P, Wp = (e->tlsc_train_w + P - 1) / P * P;
    *K0 = (int)((long long)(Hp >> level) * e->tlsc_base_h / e->tlsc_train_h);
    *K1 = (int)((long long)(Wp >> level) * e->tlsc_base_w / e->tlsc_train_w);
    return true;
}
// The step counter / coefficient row and the FiLM row a plan's sampler steps run with: a sub-batch plan's own pair, else the engine's
inline StepState* step_of(const irsde_engine* e, const Plan* pl) { return pl->own_step ? pl->own_step : e->step; }
inline float* film_of(const irsde_engine* e, const Plan* pl) { return pl->own_film ? pl->own_film : e->film_cur; }

// engine_weights.hip: weight inventory (reference state_dict names), packing into kernel layouts, FiLM rows
void build_inventory(irsde_engine* e);
void build_inventory_naf(irsde_engine* e);
void build_inventory_latent(irsde_engine* e);
void build_inventory_lpips(irsde_engine* e);
void finalize(irsde_engine* e);
void compute_film_rows(irsde_engine* e, const float* tvals, int rows, float* dst, hipStream_t s);
void ensure_film_cur(irsde_engine* e, int rows);
// the NAFBlock packing steps, shared by pack_nafblock and the kernel-level test hooks (engine_debug.hip)
void pack_conv_rows(const float* w_oihw, const float* bias, int O, int I, int KH, int KW, const std::vector<int>& perm, std::vector<float>& pw,
                    std::vector<float>& pb);                          // [O][I][KH][KW] -> [O][KH][KW][I], packed row n' = row perm[n'] (empty: identity)
std::vector<int> naf_gate_perm(int c);                               // conv4's row order: SimpleGate pairs (j, j + c) adjacent
std::vector<int> naf_shuffle_perm(int Cout);                         // ups.i.0's row order for the PixelShuffle(2) epilogue: row q * Cout / 4 + co <- co * 4 + q
std::vector<float> pack_dwconv_taps(const float* w, int c2);         // conv2.weight [2c][1][3][3] -> [9][2c]
// naf_chain_kernel's fp16 fragment streams (naf_chain_weight_halves) + fp32 vectors (naf_chain_vec_floats) of consecutive 512-channel blocks
void pack_naf_chain_host(const std::vector<NafChainHostW>& blocks, std::vector<unsigned short>& w, std::vector<float>& vecs);

// engine_plan.hip: one network evaluation as a static launch list over a static arena
Plan* get_plan(irsde_engine* e, int B, int H, int W, bool per_sample_film, int slot = 0, int b0 = 0);
int naf_subbatches(const irsde_engine* e, int B, int H, int W);
void set_force_chain_groups(int g);   // irsde_debug_force_chain_groups
void set_force_scam_stream(int block_w);   // irsde_debug_force_scam_stream (0 = the rule)
int forced_chain_groups();
int forced_scam_stream();
void set_force_subbatches(int n);                                 // irsde_debug_force_subbatches   // how many concurrent sub-batches the sampler splits a NAFNet batch into (1 = none)
LatentPlan* get_latent_plan(irsde_engine* e, int B, int H, int W, bool decode);

// engine_api.hip: runs the body of a C-ABI entry point; an exception becomes the IRSDE_ERR_* code and the thread's irsde_last_error() string
int guard(const std::function<void()>& f);
float* lpips_workspace(irsde_engine* e, int N, int H, int W);   // arch == 3: the tower's workspace for N images (grow-only)

}  // namespace irsde
