/* irsde_hip_debug.h — kernel-level TEST and TUNING hooks of libirsde_hip.so.
 *
 * Not part of the drop-in boundary (include/irsde_hip.h): nothing here replaces a reference interface.  The parity
 * tests use irsde_debug_conv to exercise one convolution code path at a time; tools/ uses irsde_bench_conv for the
 * A/B measurements logged under profiles/.  Neither changes the launch plan of an engine: the `naive` / `variant`
 * selector is turned into overrides that are handed to the launches of that one call only (no process-wide state).
 */
#ifndef IRSDE_HIP_DEBUG_H
#define IRSDE_HIP_DEBUG_H

#include "irsde_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Kernel-level test hook: one implicit-GEMM convolution (csrc/conv_igemm.hip) on NHWC device tensors.
 * in0/in1: [B][Hin][Win][C0|C1] (channel concat, in1 may be NULL); w_oihw/bias: HOST, reference layout;
 * film: device [rows][2*Cout] or NULL; res/out: device [B][Ho][Wo][Cout].  `naive` selects the code path under test:
 *   0 production dispatch      1 VALU cross-check kernel
 *   2 / 3 Winograd F(2x2,3x3) / F(4x4,3x3) (3x3 s1 p1 only); 12 / 13 and 22 / 23: the same with the component GEMMs forced
 *         onto the tile-loop kernel (all / 2 components per block)
 *   24 / 25 polyphase Winograd F(4x4,2x2) (csrc/wino.hip: wino_poly_input_kernel, the component GEMMs, wino_poly_output_kernel): 24 a 4x4 stride-2 pad-1
 *           layer (25 components, K = 4 C0), 25 a 3x3 stride-1 pad-1 layer with in_shift = 1 (4 output phases x 25 components); single source, C0 a multiple
 *           of 32, Cout of 4, bias only — anything else (film, silu, res, in1, splits > 1, another geometry) is refused
 *   48 three-launch Winograd F(4x4,3x3) on the exact-fp32 engine's three-piece GEMM (gemm_split3i_kernel: row-pair-interleaved bf16 triples, six products);
 *      26 / 27 selectors 24 / 25 on that GEMM (V written as triples by the polyphase input transform); 28: selector 27 with the transform's per-thread V
 *      writer instead of its whole-line writer (the bit-identity twin)
 *   49 a plain 1x1 layer (stride 1, no padding, C0 and C1 multiples of 32, bias only) on gemm_split3a_kernel: the weights as three bf16 pieces, the activations
 *      split inside the GEMM (csrc/gemm_split.hip); anything else is refused with the reason irsde_debug_split3_1x1_choice names
 *   46 / 47 the direct implicit GEMM on the PAIR kernels (conv_igemm.hip: fp32 storage, activations split into 16-bit hi + lo pieces while
 *           staged, three cross products on the 16-bit MFMA): fp16 / bf16 pieces
 *   44 / 45 three-launch Winograd F(4x4,3x3) with the engine's pair GEMM (pair-interleaved operands, LDS-DMA): fp16 / bf16 hi + lo pieces
 *   34 the 64-cout fused Winograd kernel (r03: Cout and C0 + C1 multiples of 64); 36: with its cout-block-by-XCD block mapping forced wherever legal;
 *      55: its production variant selected by number
 *   35 / 37 the same kernel's fp16-pair twin (IRSDE_FLAG_SPLIT_F16X2; all four hi / lo cross products on v_mfma_f32_16x16x32_f16) / with the mapping forced;
 *      56: the twin's production variant selected by number
 *   62 / 63 the two-tile-group fused Winograd kernel (r06, csrc/wino_fused_t.hip) / with the cout-block-by-XCD mapping forced wherever legal
 *   33 the fused Winograd F(4x4,3x3) kernel (csrc/wino_fused.hip; 3x3 s1 p1, H and W multiples of 4, C0, C1 and Cout multiples of 32)
 *   4 bf16-MFMA mode (halo kernel for eligible 3x3 layers); 160 / 161 its generic 256 / 128 tile
 *   5 fp16-MFMA mode (IRSDE_FLAG_FP16; halo kernel for eligible 3x3 layers); 165 its generic 128 tile
 *   204 / 260 / 261 the same three with bf16 activation storage (inputs / residual are rounded, the result widened back)
 *   162 / 262 / 166 (r05) modes 4 / 204 / 5 with the 512-pixel x 128-channel halo kernel forced (conv3x3_halo2_kernel; layers with >= 128 output channels),
 *   163 / 263 / 167 with the 256-pixel halo kernel forced
 *   100 + v: tuning variant v of the fp32 kernel: 0 production dispatch, 3 / 50 the 256x128 / 256x256 tile, 5 one block per CU, 6 generic pointer staging
 *           instead of buffer descriptors, 7 LDS-transposed instead of direct epilogue, 70 the tile-loop kernel off, 71 / 72 its batch-loop form with all / 2
 *           components per block, 73 the tile-loop kernel forced for 1x1 layers
 * Any other code is refused, 42 / 43 (the retired plane-major prototype GEMM) among them.  splits > 1 forces split-K.  Synchronises `stream`.
 * Everything of the ConvParams contract beyond bias / FiLM / SiLU / residual (in_scale, ch_scale, gate, shuffle, ln_g, fp16 storage, batched launches, knobs):
 * irsde_debug_conv_features below. */
int irsde_debug_conv(const float* in0, int C0, const float* in1, int C1, int B, int Hin, int Win, int in_shift,
                     const float* w_oihw, int Cout, int KH, int KW, int stride, int pad, const float* bias,
                     const float* film, int film_bstride, int silu, const float* res, float* out, int naive,
                     int splits, void* stream);

/* Host-only test hook: which kernel launch_conv (csrc/conv_igemm.hip: conv_validate, conv_choose) would run for one layer.  Never touches a device.
 * Geometry as for irsde_debug_conv (K x K taps; pixel strides = channel counts, out_stride = Cout).  operand: 0 f32, 1 bf16, 2 fp16 (pair != 0: the pieces'
 * type, 1 or 2).  storage: 0 f32, 1 bf16, 2 fp16 tensors on both sides.  features: bit 0 bias, 1 film, 2 silu, 3 res, 4 in_scale, 5 ch_scale, 6 gate,
 * 7 shuffle, 8 ln_g.  splits > 1: split-K with a partial buffer.  nz: components of a batched launch.  tune: a tuning code of irsde_bench_conv (0 production
 * dispatch, 3 5 6 7 50 60 61 64 65 68 69 70 - 73; 68 / 69 = 64 / 65, the halo tile order is not part of this line).  cu_count: compute units of the device to choose for.  knobs: NULL = the default tuning knobs, else 11 ints in
 * the order IRSDE_SMALL_BN, _SMALL_BN_F32, _PAIR_TILE256, _PAIR_INSCALE256, _NO_BUFA, _ZLOOP, _ZLOOP_1X1, _ZLOOP_MAXNK, _ZLOOP_MINBLK, _ZLOOP_DEEP,
 * _ZLOOP_RAGGED64 (the environment is never read).  Writes one line into out:
 *   name=<kernel> family=<n> tile=<BM>x<BN> op=<n> act=<n> inscale=<0|1> zbatch=<n> zrows=<n> grid=<x>x<y>x<z> threads=<n> lds=<bytes> row=<instance> of <rows>
 * (family: 0 pair, 1 narrow3, 2 zloop batch, 3 zloop 1x1, 4 halo, 5 igemm; op: 0 f32, 1 f32 with buffer descriptors, 2 bf16, 3 fp16; act as storage; row -1:
 * the family has no instance table; the halo path chooses its kernel and grid in csrc/conv_halo.hip: grid 0x1x1).  A layer launch_conv refuses, or a choice
 * without a kernel instance, fails with launch_conv's message. */
int irsde_debug_conv_choice(int B, int Hin, int Win, int C0, int C1, int Cout, int K, int stride, int pad, int in_shift, int operand, int storage, int pair,
                            unsigned features, int splits, int nz, int tune, int cu_count, const int* knobs, char* out, int out_len);

/* Host-only test hook: what the halo path (csrc/conv_halo.hip: conv_halo_choose) would launch for one layer that conv_choose sends to family 4.  Never touches
 * a device.  The layer as for irsde_debug_conv_choice (the CU count and the knobs do not reach this choice).  tune: 0 the production rules, 64 / 65 the
 * 512- / 256-pixel kernel forced, 68 / 69 the same two with the output-channel blocks running slowest wherever the layer has more than one.  halo2, nslow: the
 * values of IRSDE_HALO2 and IRSDE_HALO_NSLOW to choose under (the defaults are 1 and -1; the environment is never read).  Writes one line into out:
 *   kernel=halo256|halo512 bn=<64|128> op=<2|3> act=<0|1> tiles=<x>x<y> nblk_n=<n> nslow=<0|1> grid=<n> lds=<bytes> instance=<i> of 9
 * (instance: conv3x3_halo_bf16_kernel<128> / <64> on f32 tensors, on bf16 tensors, with fp16 operands, then conv3x3_halo2_kernel in the same three forms).
 * A layer launch_conv refuses fails with its message, a layer of another family with one that names the family's kernel. */
int irsde_debug_conv_halo_choice(int B, int Hin, int Win, int C0, int C1, int Cout, int K, int stride, int pad, int in_shift, int operand, int storage, int pair,
                                 unsigned features, int splits, int nz, int tune, int halo2, int nslow, char* out, int out_len);

/* Kernel-level test hook: ONE production launch_conv (csrc/conv_igemm.hip) with the whole ConvParams contract, in irsde_debug_conv_choice's language.
 * Geometry as for irsde_debug_conv (NHWC device tensors, in0 / in1 concat, in_shift, K x K taps).  operand / storage / pair as for irsde_debug_conv_choice; with
 * 16-bit storage the caller's fp32 in0 / in1 / res are rounded on the device into bf16 / fp16 copies of the same extents and the 16-bit result (pre-filled with
 * NaN) is widened back into out.  HOST, reference layout: w_oihw [nz][Cout][C0 + C1][K][K], bias / ch_scale / ln_g [Cout] (NULL = absent) — packed by the
 * engine's own functions: pack_conv_rows with naf_gate_perm (gate) or naf_shuffle_perm (shuffle), launch_split_pairs + pow2_scale_into_512 (pair).  DEVICE:
 * film [rows][2 Cout] with film_bstride, res, in_scale [B][C0], gate_film [B][Cout / 2 scales | Cout / 2 shifts] with gate_film_bstride.  Epilogue: bias -> FiLM ->
 * SiLU -> ch_scale -> one of: gate (out [B][Ho][Wo][Cout / 2] = v[j] v[j + Cout / 2], then gate_film: (.)(s + 1) + t), shuffle (out and res [B][2Ho][2Wo][Cout / 4]:
 * PixelShuffle(2), then + res), ln_g (after the bias: channel LayerNorm, gain ln_g, eps 1e-5, then + res), else + res (out and res [B][Ho][Wo][Cout]).
 * nz > 1: a batched launch of nz 1x1 GEMMs (B = 1, Hin = 1, K = 1, one fp32 source): in0 [nz][Win][C0], w [nz][Cout][C0], out [nz][Win][Cout].
 * splits / tune / knobs as for irsde_debug_conv_choice; the knobs are handed to this one launch (no process-wide state).  choice receives
 * irsde_debug_conv_choice's line for the choice the launch made (the launch's own ConvChoice; the device's CU count); a launch of family 4 appends the fields of
 * irsde_debug_conv_halo_choice's line for its own HaloChoice (tune 64 / 65: the 512- / 256-pixel halo kernel forced, 68 / 69: the same with the
 * output-channel blocks slowest).  Refused before anything is launched:
 * whatever conv_validate refuses, nz > 1 with another geometry, gate with shuffle / res / film, shuffle with film, gate_film without gate.  Tensors are
 * used at their exact extents.  Synchronises `stream`.  tests/test_gpu_conv_rows.py compares it with tests/conv_rows_oracle.py. */
int irsde_debug_conv_features(const float* in0, int C0, const float* in1, int C1, int B, int Hin, int Win, int in_shift, const float* w_oihw, int Cout, int K,
                              int stride, int pad, int operand, int storage, int pair, const float* bias, const float* ch_scale, const float* ln_g,
                              const float* film, int film_bstride, const float* res, const float* in_scale, const float* gate_film, int gate_film_bstride,
                              int silu, int gate, int shuffle, int nz, int splits, int tune, const int* knobs, float* out, char* choice, int choice_len,
                              void* stream);

/* Kernel-level test hook of csrc/gemm_split.hip: C_z[M][N] = A_z[M][K] . B_z[N][K]^T for z < ncomp (device f32 tensors, z-major),
 * operands split into 16-bit pieces on the device (nplanes = 42 / 44: the engine's
 * pair-interleaved two-piece kernel with bf16 / fp16 pieces; nplanes = 43: the exact-fp32 engine's three-piece kernel gemm_split3i_kernel, six products, on
 * its production launch — at most one block per compute unit, each walking several (component, row tile, column tile) items; nplanes = 45: the same kernel
 * with one item per block, the walk's bit-identity twin; nplanes = 47: the production launch with s_waitcnt vmcnt(0) in front of every barrier of the K loop,
 * the bit-identity twin of the kernel's load ring), products on the 16-bit MFMA, f32 accumulate.  K a multiple of 32.  Any other nplanes is refused, 2 / 3 (the
 * retired plane-major prototype kernel) among them.  Synchronises `stream`. */
int irsde_debug_split_gemm(const float* A, const float* B, float* C, int M, int N, int K, int ncomp, int nplanes, void* stream);

/* Kernel tuning hook: average ms of one KxK convolution (pad K/2, or 4x4 s2 p1) on random NHWC data.  variant (any other code is refused, 412 / 413 / 422 / 423
 * of the retired plane-major prototype GEMM among them):
 *   0 production dispatch, 3 / 50 fp32 256x128 / 256x256 tiles, 5 one block per CU, 6 generic pointer staging instead of buffer descriptors,
 *     7 LDS-transposed instead of direct epilogue, 70 the tile-loop kernel off, 71 / 72 its batch-loop form with all / 2 components per block, 73 forced for 1x1 layers
 *   60 / 61 / 62 bf16 mode (256 tile / 128 tile / automatic incl. the halo kernel), 63 = 62 with bf16 activation storage,
 *     64 / 65 = 62 and 66 / 67 = 63 with the 512- / 256-pixel halo kernel forced (r05)
 *   80 / 81 Winograd F(4x4,3x3) fused kernel / three-launch path (3x3 s1 only), 82 the fused kernel once with its phase timeline printed to stdout,
 *     82 + f (f in 1..255) the fused kernel with tuning-aid flags f (1 no patch traffic, 2 no weight traffic, 4 / 8 producer / MFMA waves at raised priority)
 *   421 the three-launch path's native f32 component GEMMs alone
 *   430 the 64-cout fused Winograd kernel (r04 persistent form, production), 431 / 432 its weight fragments / patch loads read zeros, 434 its fp16-pair twin,
 *     435 (= 2004) the kernel once with its per-wave cycle budget printed to stdout, 2001 / 2002 that stamp run without weight / patch traffic
 *   460 the two-tile-group fused Winograd kernel (r06, production), 461 / 462 its weight fragments / patch gathers read zeros, 467 / 468 / 469 without
 *     transform arithmetic / also without gathers / without gathers only, 465 the kernel once with its per-wave cycle stamps printed to stdout,
 *     4650 / 4651 / 4652 that stamp run without patch traffic / output stores / residual loads, 4653 the stamps of the coalesced-epilogue twin (PROBES build)
 *   472 the engine's pair-interleaved two-plane GEMM alone, 473 / 475 / 476 without its global loads / MFMAs / output stores (474: no such twin, the launch refuses it)
 *   490 the three-piece GEMM (gemm_split3i_kernel) alone on the layer's 36 F(4x4,3x3) component shapes, 491 / 493 / 494 without its global loads / MFMAs /
 *     output stores (PROBES build; 492: no such twin, the launch refuses it); 495 - 499: the same five on the one-item-per-block launch (the walk's twin)
 *     500 - 504: the same five on the drain twin (vmcnt(0) in front of every barrier of the K loop: what the load ring's span across barriers buys)
 *   510 a plain 1x1 layer (K = 1, stride 1, epi 0) on gemm_split3a_kernel alone, 511 / 513 / 514 without its global loads / MFMAs / output stores (PROBES
 *     build; 512: no such twin); 515 - 519: the same five on the one-item-per-block launch; 520 - 524: on the drain twin
 *   480 / 481 / 482 a direct layer on the PAIR kernels (fp16 / bf16 pieces / fp16 without the 256 x 256 tile)
 * epi: 0 none, 1 FiLM+SiLU, 2 SiLU+residual. */
int irsde_bench_conv(int variant, int B, int H, int W, int Cin, int Cout, int K, int stride, int up, int epi, int iters,
                     double* ms_out);
/* Times naf_chain_kernel (csrc/naf_chain.hip) alone on synthetic data: `nblocks` consecutive 512-channel NAFBlocks on B images of 8 x 8 pixels,
 * `iters` launches; variant 1 residual stream in registers + ring of 8 weight fragments (= 0, production), 2 residual stream in L2 + ring of 16,
 * 22 / 24 the kernel on 2 / 4 work-groups per image (r06; 25, PROBES build: 24 + its per-phase cycle stamps; 26, PROBES build: 24 with one group per image missing — the call must fail with the spin timeout).
 * *ms_out = milliseconds per launch.  (tools/naf_chain_bench.py) */
int irsde_bench_naf_chain(int variant, int nblocks, int B, int iters, double* ms_out);
/* Test / measurement hook (process-wide): the number of concurrent sub-batches irsde_sample splits a ConditionalNAFNet batch into — n >= 1 forces it
 * (1 = never split; clipped to 4 and to a divisor of the batch), 0 returns to the heuristic (2 parts from 8 images on (r06; r05: 64), and only where a level
 * runs as a NAFBlock chain).  Plans are cached per split, so changing it never invalidates anything. */
int irsde_debug_force_subbatches(int n);
/* Test / measurement hook (process-wide): work-groups per image of the NAFBlock chain kernel in plans built from now on — 1 the one-group kernel, 2 / 4
 * forced (where 8 ceil(B / 8) g groups fit the compute units next to the call's other sub-batches, else fewer), 0 returns to the rule (as many as fit).
 * Plans already built keep their choice: use a fresh engine (or another batch shape) per setting. */
int irsde_debug_force_chain_groups(int g);
/* Test / measurement hook (process-wide): the polyphase Winograd F(4x4,2x2) path of the resampling convolutions in engines CREATED from now on (the
 * weights are transformed at irsde_finalize_weights) — 0 never, 1 by the plan's rule, 2 wherever eligible (exact fp32, single source, bias only);
 * any other value returns to the default (the rule; the IRSDE_WINO_POLY tuning knob). */
int irsde_debug_force_wino_poly(int mode);
/* Test / measurement hook (process-wide): the three-piece bf16 component GEMMs of the exact-fp32 engine in engines CREATED from now on (the weights' triples
 * are made at irsde_finalize_weights) — 0 never, 1 by the plan's rule, 2 wherever eligible (exact fp32, K a multiple of 32, 32-bit component offsets);
 * any other value returns to the default (the rule; the IRSDE_SPLIT3 tuning knob).  IRSDE_FLAG_NO_SPLIT3 wins over every mode. */
int irsde_debug_force_split3(int mode);
/* Test / measurement hook (process-wide): the three-piece bf16 projections of the exact-fp32 engine's fused LinearAttention blocks (C = 64 / 128 / 256) in plans
 * BUILT from now on — 0 never, 1 by the plan's rule, 2 wherever a kernel instance exists; any other value returns to the default (the rule; the IRSDE_SPLIT3_ATTN
 * tuning knob).  IRSDE_FLAG_NO_SPLIT3 and irsde_debug_force_split3(0) win over every mode; irsde_debug_force_split3(2) does not force it. */
int irsde_debug_force_split3_attn(int mode);
/* Test / measurement hook (process-wide, read at every launch): caps the grid of the three-piece GEMM's persistent launch at n blocks, n >= 8 (one per XCD),
 * so that a small problem makes every block walk several items; a negative n returns to the default (one block per compute unit).  0 .. 7: IRSDE_ERR_INVALID,
 * nothing changes.  Results do not depend on it (tests/test_gpu_split3_walk.py). */
int irsde_debug_force_split3_blocks(int n);
/* Test / measurement hook (process-wide): the plain 1x1 convolutions of the exact-fp32 engine on three bf16 pieces (gemm_split3a_kernel) in plans BUILT from
 * now on — 0 never, 1 by the plan's rule, 2 wherever eligible; any other value returns to the default (the rule; the IRSDE_SPLIT3_1X1 tuning knob).
 * IRSDE_FLAG_NO_SPLIT3 and irsde_debug_force_split3(0) win over every mode; irsde_debug_force_split3(2) does not force it. */
int irsde_debug_force_split3_1x1(int mode);
/* Kernel-level test hook of gemm_split3a_kernel (csrc/gemm_split.hip): out[m][n] = sum_k A[m][k] w[n][k] (+ bias[n]) with A = up to two f32 sources side by
 * side (in0: C0 channels at pixel stride pix0; in1: C1, pix1, or NULL with C1 = 0; C0, C1 multiples of 32), w [N][C0 + C1] f32, bias [N] or NULL, out at row
 * stride out_stride >= N — all DEVICE pointers.  w is split into three bf16 pieces on the device, the activations inside the kernel: bit-identical to
 * irsde_debug_split_gemm(nplanes 43) on the concatenated A.  mode: 0 the production walk, 1 one item per block, 2 the walk with vmcnt(0) in front of every
 * barrier of the K loop (the bit-identity twins).  irsde_debug_force_split3_blocks caps this walk's grid too.  Synchronises `stream`. */
int irsde_debug_split3_1x1(const float* in0, int C0, int pix0, const float* in1, int C1, int pix1, const float* w, const float* bias, float* out, int M, int N,
                           int out_stride, int mode, void* stream);
/* Host-only test hook: does a layer run on gemm_split3a_kernel (split3_1x1_choose)?  Never touches a device, never reads the environment.  The layer as for
 * irsde_debug_conv_choice; engine_flags: the engine's IRSDE_FLAG_* word; master: the mode of IRSDE_SPLIT3 / irsde_debug_force_split3; knob: the mode of
 * IRSDE_SPLIT3_1X1; cu_count: compute units.  Writes one line into out:
 *   adopt=<0|1> grid=<blocks> lds=<bytes> why_not=<the first reason of a refusal, empty when adopted> */
int irsde_debug_split3_1x1_choice(int B, int Hin, int Win, int C0, int C1, int Cout, int K, int stride, int pad, int in_shift, int operand, int storage, int pair,
                                  unsigned features, int splits, int nz, int engine_flags, int master, int knob, int cu_count, char* out, int out_len);

/* Kernel-level test hook: ONE SCAM of the stereo-sr NAFBlock (csrc/scam.hip + the projection GEMM on the implicit-GEMM kernel, the engine's
 * fp32 path).  x / out: device NHWC [2 B_pairs][H][W][C] (views stacked [L_0..L_{B-1}, R_0..R_{B-1}] as inside the reference network);
 * every weight is a HOST pointer in reference layout: norm_*_g [C], *_proj*_w [C][C] (1x1), *_proj*_b [C], beta / gamma [C].
 * C a multiple of 32 in [32, 1024], H and W >= 4, W / 4 <= 512.  Synchronises `stream`. */
int irsde_debug_scam(const float* x, int B_pairs, int H, int W, int C, const float* norm_l_g, const float* norm_r_g, const float* l_proj1_w,
                     const float* l_proj1_b, const float* r_proj1_w, const float* r_proj1_b, const float* l_proj2_w, const float* l_proj2_b,
                     const float* r_proj2_w, const float* r_proj2_b, const float* beta, const float* gamma, float* out, void* stream);

/* Kernel-level test hooks of the NAFBlock glue kernels (csrc/kernels_misc.hip, csrc/tlsc_pool.hip): each runs the production launchers of ONE
 * stage on the caller's device tensors (NHWC fp32) and synchronises `stream`.  Weights are HOST pointers in reference layout and go through the engine's own
 * packing (engine_weights.hip); FiLM / scale rows and activations are DEVICE pointers.  A shape a launcher cannot run is refused before anything is launched.
 * tests/test_gpu_naf_glue.py compares them with tests/naf_glue_oracle.py.
 *
 * conv2 (depthwise 3x3, pad 1) + SimpleGate + SCA: launch_dwconv_gate, then launch_sca (one launch while tiles * c <= 65536, else mean + sca.1 kernels).
 * u [B][H][W][2c]; conv2_w [2c][1][3][3], conv2_b [2c], sca_w [c][c], sca_b [c]; gated_out [B][H][W][c]; s_out [B][c] = sca.1(mean(gated));
 * mean_out [B][c] (may be NULL): the pooled mean itself, formed from the gate kernel's tile partials by the mean kernel on either route.
 * c a multiple of 4, B <= 65535. */
int irsde_debug_naf_gate_sca(const float* u, int B, int H, int W, int c, const float* conv2_w, const float* conv2_b, const float* sca_w, const float* sca_b,
                             float* gated_out, float* mean_out, float* s_out, void* stream);
/* TLSC: launch_tlsc_pool of g [B][h][w][c] over k1 x k2 windows -> pooled_out [B][h - k1 + 1][w - k2 + 1][c] (window means); then scaled_out = g (a copy)
 * times the caller's scale_map (device, pooled_out's shape) replicate-padded to h x w by launch_tlsc_scale.  c a multiple of 4, 1 <= k1 <= h, 1 <= k2 <= w. */
int irsde_debug_tlsc(const float* g, int B, int h, int w, int c, int k1, int k2, float* pooled_out, const float* scale_map, float* scaled_out, void* stream);
/* Channel LayerNorm + FiLM: launch_layernorm_film.  x / out [M][C], image of pixel m = m / ppi; g [C] HOST; fscale / fshift: DEVICE rows of C floats,
 * row of image b at + b * film_bstride (0: one shared row); out = LN(x) * g * (fscale + 1) + fshift.  C a multiple of 4 in [4, 2048], film_bstride a multiple of 4. */
int irsde_debug_ln_film(const float* x, long long M, int C, long long ppi, const float* g, const float* fscale, const float* fshift, int film_bstride,
                        float* out, void* stream);
/* naf_lnconv_kernel (fp16 operand mode; c in {64, 128, 256}, Cout a multiple of 64) in its three prologues.  x [M][c]; w [Cout][c] and bias [Cout] HOST
 * (rounded to fp16 on the device like an engine's copy); mode
 *   0  launch_naf_lnconv: out [M][Cout] = W fp16(LN(x) g (fscale + 1) + fshift) + bias       (norm1 + conv1)
 *   1  the same with the SimpleGate epilogue (w rows interleaved like a packed conv4): out [M][Cout / 2] = v[j] v[j + Cout / 2], then, with gate_film
 *      (DEVICE, per image [scale (Cout / 2) | shift (Cout / 2)], row stride gate_film_bstride; may be NULL), * (scale + 1) + shift   (norm2 + conv4)
 *   2  launch_naf_pwconv: out [M][Cout] = res + (W fp16(x * in_scale[image]) + bias) * ch_scale  (conv3; in_scale DEVICE [images][c])
 *   3  the same without in_scale (conv5; in_scale is ignored)
 * g [c] (modes 0 / 1) and ch_scale [Cout] (modes 2 / 3) HOST; fscale / fshift as in irsde_debug_ln_film; res DEVICE [M][Cout].  Arguments a mode does not
 * use may be NULL. */
int irsde_debug_naf_lnconv(int mode, const float* x, long long M, int c, int Cout, long long ppi, const float* g, const float* fscale, const float* fshift,
                           int film_bstride, const float* w, const float* bias, const float* gate_film, int gate_film_bstride, const float* in_scale,
                           const float* ch_scale, const float* res, float* out, void* stream);

/* naf_chain_kernel (csrc/naf_chain.hip): `nblocks` consecutive 512-channel NAFBlocks on B images of 8 x 8 pixels as ONE launch of the production launcher —
 * groups == 1: launch_naf_chain; groups == 2 / 4: naf_chain_build_split_weights + launch_naf_chain_split on a freshly zeroed scratch buffer.
 * x / out: DEVICE [B][64][512] fp32 (NHWC).  The sixteen weight arguments are HOST pointers in reference layout, each holding `nblocks` consecutive tensors
 * (norm1.g [512], conv1.weight [1024][512], conv1.bias [1024], conv2.weight [1024][1][3][3], conv2.bias [1024], sca.1.weight [512][512], sca.1.bias [512],
 * conv3.weight [512][512], conv3.bias [512], beta [512], norm2.g [512], conv4.weight [1024][512], conv4.bias [1024], conv5.weight [512][512], conv5.bias [512],
 * gamma [512]); they go through the engine's own packing (pack_naf_chain_host).  film: DEVICE, the row of image b at + b * film_bstride (0: one shared row),
 * block i at + film_off + i * 2048 = [shift_att | scale_att | shift_ffn | scale_ffn]; cam: DEVICE or NULL, row b at + b * cam_bstride, block i at
 * + cam_off + i * 1024 = [scale | shift].  Strides and offsets are multiples of 4.  Refused before anything is launched: groups other than 1 / 2 / 4,
 * more work-groups (8 ceil(B / 8) groups) than compute units, nblocks < 1.  groups > 1: the call launches ONCE; if the kernel raised its error word the
 * call fails naming the co-residency (spin) timeout, and it fails if a barrier counter was not restored to zero.  Synchronises `stream`.
 * tests/test_gpu_naf_chain.py compares it with tests/naf_chain_oracle.py. */
int irsde_debug_naf_chain(const float* x, float* out, int B, int nblocks, const float* norm1_g, const float* conv1_w, const float* conv1_b, const float* conv2_w,
                          const float* conv2_b, const float* sca_w, const float* sca_b, const float* conv3_w, const float* conv3_b, const float* beta,
                          const float* norm2_g, const float* conv4_w, const float* conv4_b, const float* conv5_w, const float* conv5_b, const float* gamma,
                          const float* film, int film_bstride, int film_off, const float* cam, int cam_bstride, int cam_off, int groups, void* stream);
/* Host only: naf_chain_split_order(nblocks, groups) — for every 1 KB fragment of the groups-per-image weight streams its position in the one-group
 * streams — into order_out[n], n = 8 * nblocks * 448 (any other n is refused). */
int irsde_debug_naf_chain_split_order(int nblocks, int groups, int* order_out, long long n);

/* Kernel-level test hook: the full softmax attention core of the denoising-sde bottleneck on bf16 tensors (csrc/full_attn16.hip, IRSDE_FLAG_BF16_ACT) —
 * ONE launch of the production launcher on the caller's device tensors: qkv_bf16 [B][N][384] (rows q | k | v, 4 heads x 32) -> out_bf16 [B][N][128], both
 * bf16 and 16-byte aligned.  B, N >= 1, 4 B <= 65535.  Rows behind row N of `out` are not written.  Synchronises `stream`.
 * tests/test_gpu_dsde_unet16.py compares it with tests/dsde_unet16_oracle.py. */
int irsde_debug_full_attention16(const void* qkv_bf16, int B, int N, void* out_bf16, void* stream);

/* Kernel-level test hooks of csrc/linear_attn.hip (tests/test_gpu_linear_attn.py compares them with tests/linear_attn_oracle.py; outside the drop-in boundary,
 * irsde_version() unchanged).  Activations are DEVICE tensors in NHWC order with the pixels flattened ([B][N][channels]), weights HOST pointers in reference
 * layout.  B in [1, 16383]; N a positive multiple of 4 (the least a network level produces), anything else is refused.  The chunk workspace is sized as
 * Builder::attn_workspace sizes it and starts as NaN.  Rows behind row N of an output are not written.  Both synchronise `stream`.
 *
 * irsde_debug_attn_block: ONE Residual(PreNorm(LinearAttention)) on the fused route of Builder::attn — launch_attention_kv_context (PreNorm's LayerNorm, k / v
 * projection, context) and launch_attention_q_out_fused (LayerNorm, q projection, softmax, context product, to_out, LayerNorm, residual), nothing else.
 * x / y [B][N][C] fp32; norm_g = norm.g [C], to_qkv_w = to_qkv.weight [384][C], to_out_w = to_out.0.weight [C][128], to_out_b = to_out.0.bias [C],
 * to_out_g = to_out.1.g [C].  mode: AttnMode by number (0 f32, 1 fp16 hi + lo pairs, 2 bf16, 3 fp16, 4 three bf16 pieces); the mode's weight planes are made by
 * the functions behind the engine's own copies (launch_f32_to_bf16 / launch_f32_to_f16, launch_split_planes with pow2_scale_into_512, launch_split_frag3).
 * act_bf16 (mode 2 only): x is rounded into a bf16 copy on the device, the kernels read and write bf16 tensors, the bf16 result (pre-filled with NaN) is widened
 * back into y.  A (C, mode, act_bf16) without a row in either instance table is refused with the launcher's message before anything is launched. */
int irsde_debug_attn_block(const float* x, int B, int N, int C, const float* norm_g, const float* to_qkv_w, const float* to_out_w, const float* to_out_b,
                           const float* to_out_g, int mode, int act_bf16, float* y, void* stream);
/* irsde_debug_attn_core: the attention core alone on the two routes that have a tensor in front of it; out [B][N][128] (heads x 32 channels).
 *   route 1  Builder::attn's fused_kv route: in = xn [B][N][C], ALREADY normalised; wkv = the k | v rows of to_qkv.weight ([256][C], HOST); q = DEVICE [B][N][128]
 *            (the q convolution's output).  launch_attention_kv_context without ln_g (fp32, C a multiple of 32 up to 256), then launch_attention_q_out.  bf16 = 0.
 *   route 2  in = q | k | v [B][N][384] (wkv, q: NULL; C is ignored): launch_linear_attention.  bf16 != 0: the tensor is rounded into a bf16 copy, the kernels run
 *            on bf16 storage, the result (pre-filled with NaN) is widened back.
 * The q convolution, to_out and its LayerNorm are convolutions / glue that other hooks cover. */
int irsde_debug_attn_core(int route, const float* in, int B, int N, int C, const float* wkv, const float* q, int bf16, float* out, void* stream);
/* Host only (never touches a device, never reads the environment): what the two fused launchers read for (C, mode, act_bf16) on B images of N pixels — their
 * instance tables and attn_chunk_len / attn_num_chunks.  Writes one line into out:
 *   kv_row=<i|-1> of 23 qo_row=<i|-1> of 18 kv_lds=<bytes> qo_lds=<bytes> kv_tile=<px> qo_tile=<px> chunk_len=<px> nch=<n>
 * (row -1, lds 0: the table has no such instance; `of` = the tables' lengths).  The three-pass kernels of route 2 use chunk_len and nch alone. */
int irsde_debug_attn_choice(int C, int mode, int act_bf16, int N, int B, char* out, int out_len);

/* Kernel-level test hook: ONE full-resolution SCAM of the stereo-sr ConditionalUNet (csrc/scam.hip *_full kernels + the projection GEMM on the
 * implicit-GEMM kernel, fp32) — the counterpart of irsde_debug_scam, same argument order.  x / out: device NHWC [2 B_pairs][H][W][C], views stacked
 * [L_0..L_{B-1}, R_0..R_{B-1}]; every weight is a HOST pointer in reference layout.  C a multiple of 32 in [32, 2048], H, W >= 1, W <= 1024
 * (wider: IRSDE_ERR_INVALID).  Synchronises `stream`. */
int irsde_debug_scam_full(const float* x, int B_pairs, int H, int W, int C, const float* norm_l_g, const float* norm_r_g, const float* l_proj1_w,
                          const float* l_proj1_b, const float* r_proj1_w, const float* r_proj1_b, const float* l_proj2_w, const float* l_proj2_b,
                          const float* r_proj2_w, const float* r_proj2_b, const float* beta, const float* gamma, float* out, void* stream);

/* Kernel-level test hooks: irsde_debug_scam / irsde_debug_scam_full with the streaming core (csrc/scam_stream.hip, what IRSDE_FLAG_SCAM_STREAM runs on rows
 * beyond the strip kernels' width) between the same prologue, projections and epilogue — same arguments plus block_w before `out`: the column block of the
 * online softmax, a multiple of 16 in [16, 512], or 0 for the default (512).  Any width; B_pairs * H' <= 65535 (H' = H / 4 for irsde_debug_scam_stream,
 * H for irsde_debug_scam_full_stream); the channel limits of their counterparts.  Synchronise `stream`.  tests/test_gpu_scam_stream.py. */
int irsde_debug_scam_stream(const float* x, int B_pairs, int H, int W, int C, const float* norm_l_g, const float* norm_r_g, const float* l_proj1_w,
                            const float* l_proj1_b, const float* r_proj1_w, const float* r_proj1_b, const float* l_proj2_w, const float* l_proj2_b,
                            const float* r_proj2_w, const float* r_proj2_b, const float* beta, const float* gamma, int block_w, float* out, void* stream);
int irsde_debug_scam_full_stream(const float* x, int B_pairs, int H, int W, int C, const float* norm_l_g, const float* norm_r_g, const float* l_proj1_w,
                                 const float* l_proj1_b, const float* r_proj1_w, const float* r_proj1_b, const float* l_proj2_w, const float* l_proj2_b,
                                 const float* r_proj2_w, const float* r_proj2_b, const float* beta, const float* gamma, int block_w, float* out,
                                 void* stream);
/* Test / measurement hook (process-wide): block_w a multiple of 16 in [16, 512] — plans built from now on run EVERY SCAM core of the stereo networks on the
 * streaming kernel with that block width, whatever the row width and the engine's flags (how small networks exercise several blocks per row); 0 returns to the
 * rule (IRSDE_FLAG_SCAM_STREAM and a row beyond the strip limit).  Any other value: IRSDE_ERR_INVALID, nothing changes.  Plans already built keep their
 * choice: use a fresh engine per setting. */
int irsde_debug_force_scam_stream(int block_w);

/* Kernel-level test hook: the ReLU'd feature map of ONE tap (1..5) of the LPIPS tower (csrc/lpips.hip: prologue, convolutions, max-pools) on an engine of
 * irsde_create_lpips with finalized weights.  in: device NCHW fp32 [B][3][H][W], scaled as irsde_lpips scales it (normalize as there); dst: device NHWC
 * [B][h][w][C] of the tap, or NULL to query dims only; dims receives {B, h, w, C}.  H, W >= 31.  Synchronises `stream`.  tests/test_gpu_lpips.py compares
 * it with tests/lpips_oracle.py. */
int irsde_debug_lpips_tap(irsde_engine* e, const float* in, int B, int H, int W, int normalize, int tap, float* dst, int64_t dims[4], void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IRSDE_HIP_DEBUG_H */
