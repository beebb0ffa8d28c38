// libirsde_hip.so — the kernel-level TEST and TUNING hooks (include/irsde_hip_debug.h): one kernel or one code path at a time on the caller's or on
// synthetic data.  Not part of the drop-in boundary; nothing here touches an engine.  Device memory, the hook's stream and its events are scoped
// (Scratch, OwnedStream, EventPair): every early return and every throw releases them.
#include "engine.h"
#include "../../include/irsde_hip_debug.h"

using namespace irsde;

namespace irsde {
namespace {

// Device scratch of one hook call on stream `s`: freed, after `s` has drained, however the call ends
struct Scratch {
    hipStream_t s;
    std::vector<void*> bufs;
    explicit Scratch(hipStream_t s_) : s(s_) {}
    ~Scratch() {
        (void)hipStreamSynchronize(s);
        for (void* p : bufs) (void)hipFree(p);
    }
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    template <class T> T* alloc(size_t n) {
        void* p = nullptr;
        IRSDE_HIP_CHECK(hipMalloc(&p, n * sizeof(T)));
        bufs.push_back(p);
        return static_cast<T*>(p);
    }
    float* upload(const float* host, size_t n) {
        float* d = alloc<float>(n);
        IRSDE_HIP_CHECK(hipMemcpy(d, host, n * sizeof(float), hipMemcpyHostToDevice));
        return d;
    }
    float* upload(const std::vector<float>& v) { return upload(v.data(), v.size()); }
};
// The stream a bench hook runs on (declare it before the Scratch that drains it)
struct OwnedStream {
    hipStream_t s = nullptr;
    explicit OwnedStream(unsigned flags) { IRSDE_HIP_CHECK(hipStreamCreateWithFlags(&s, flags)); }
    ~OwnedStream() { (void)hipStreamDestroy(s); }
    OwnedStream(const OwnedStream&) = delete;
    OwnedStream& operator=(const OwnedStream&) = delete;
};
struct EventPair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    EventPair() {
        IRSDE_HIP_CHECK(hipEventCreate(&e0));
        IRSDE_HIP_CHECK(hipEventCreate(&e1));
    }
    ~EventPair() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    EventPair(const EventPair&) = delete;
    EventPair& operator=(const EventPair&) = delete;
};
// milliseconds per call of `iters` calls of run() on `s`, between two events
template <class Run>
double time_launches(hipStream_t s, int iters, Run&& run) {
    EventPair ev;
    IRSDE_HIP_CHECK(hipEventRecord(ev.e0, s));
    for (int i = 0; i < iters; ++i) run();
    IRSDE_HIP_CHECK(hipEventRecord(ev.e1, s));
    IRSDE_HIP_CHECK(hipStreamSynchronize(s));
    float ms = 0.f;
    IRSDE_HIP_CHECK(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    return ms / iters;
}

// ---------------------------------------------------------------------------------------------------------------
// The selector codes of irsde_debug_conv / irsde_bench_conv (include/irsde_hip_debug.h documents them).  A code is looked up ONCE, in the tables below; a code
// without a row is refused, never run as the production dispatch.  The numbers live here and nowhere else.
// ---------------------------------------------------------------------------------------------------------------

// launch_conv's tuning codes (irsde_bench_conv's small variants; irsde_debug_conv 100 + code) -> the overrides of that one call.  Every code but 0 also
// switches the grid-filling rules off.  50 belongs to the f32 kernels, 60 / 61 to the 16-bit-operand and PAIR kernels (with the halo kernel out of the way).
ConvTune conv_tune_from_code(int code) {
    ConvTune t;
    t.rules_off = code != 0;
    switch (code) {
        case 3: t.tile = ConvTune::TILE_256x128; break;
        case 50: t.tile = ConvTune::TILE_256; break;
        case 5: t.tile = ConvTune::TILE_128_ONE_PER_CU; break;
        case 6: t.no_buffer_desc = true; break;
        case 7: t.no_direct_epi = true; break;
        case 60: t.tile = ConvTune::TILE_256; t.halo = ConvTune::HALO_OFF; break;
        case 61: t.tile = ConvTune::TILE_128; t.halo = ConvTune::HALO_OFF; break;
        case 64: t.halo = ConvTune::HALO_FORCE_512; break;
        case 65: t.halo = ConvTune::HALO_FORCE_256; break;
        case 68: t.halo = ConvTune::HALO_FORCE_512; t.halo_order = ConvTune::ORDER_N_SLOW; break;   // (66 / 67 are irsde_bench_conv's own variants)
        case 69: t.halo = ConvTune::HALO_FORCE_256; t.halo_order = ConvTune::ORDER_N_SLOW; break;
        case 70: t.zloop = ConvTune::ZLOOP_OFF; break;
        case 71: t.zloop = ConvTune::ZLOOP_ALL; break;
        case 72: t.zloop = ConvTune::ZLOOP_PAIRS; break;
        case 73: t.zloop = ConvTune::ZLOOP_FORCE_1X1; break;
        default: break;
    }
    return t;
}

// The three-piece GEMM's launch twins: 0 the production launch (the tuning knobs apply), 1 one item per block, 2 the walk's drain twin — irsde_debug_split_gemm
// 43 / 45 / 47 in that order, irsde_bench_conv 490 + 5 twin + abl (abl: Split3Launch::Abl by number; one the kernel lacks is refused by the launcher)
Split3Launch split3_launch_twin(int twin, int abl = 0) {
    Split3Launch o;
    o.abl = static_cast<Split3Launch::Abl>(abl);
    o.walk = twin == 0 ? Split3Launch::RULE : twin == 1 ? Split3Launch::OFF : Split3Launch::ON;
    o.drain = twin == 0 ? Split3Launch::RULE : twin == 1 ? Split3Launch::OFF : Split3Launch::ON;
    return o;
}

enum class Operand { F32, BF16, F16 };

enum class ConvPath {
    Direct,        // launch_conv: operand mode, bf16 activation storage, tuning code
    Valu,          // the VALU cross-check kernel
    WinoF2,        // three-launch Winograd F(2x2,3x3) on the f32 GEMM: tuning code
    WinoF4,        // the same, F(4x4,3x3)
    Poly,          // polyphase F(4x4,2x2) on the f32 GEMM: up
    PolyTriples,   // polyphase on the three-piece GEMM: up, thread writer
    F4Triples,     // three-launch F(4x4,3x3) on the three-piece GEMM
    F4Pairs,       // three-launch F(4x4,3x3) on the pair GEMM: fp16 / bf16 pieces
    DirectPair,    // launch_conv on the PAIR kernels: fp16 / bf16 pieces
    Fused32,       // wino_fused.hip, 32 couts per block
    Fused64,       // 64 couts per block: launch variant
    Fused64Pair,   // its fp16-pair twin: launch variant
    Fused64T,      // wino_fused_t.hip, two tile groups: launch variant
    Split3a,       // a plain 1x1 layer on gemm_split3a_kernel (three bf16 pieces, the activations split inside the GEMM)
};
struct DebugConvRow {
    int code;
    ConvPath path;
    Operand op;
    bool act_bf16;        // bf16 activation storage (IRSDE_FLAG_BF16_ACT): inputs / residual are rounded, the result widened back
    int tune;             // conv_tune_from_code
    int variant;          // the variant int of launch_wino_fused64 / launch_wino_fused64t
    bool up;              // polyphase: the 3x3 layer behind the nearest x2 upsample (else the 4x4 stride-2 layer)
    bool thread_writer;   // polyphase on triples: the per-thread V writer
};
constexpr DebugConvRow direct(int code, Operand op, bool act_bf16, int tune) { return {code, ConvPath::Direct, op, act_bf16, tune, 0, false, false}; }
constexpr DebugConvRow on_path(int code, ConvPath path, Operand op = Operand::F32) { return {code, path, op, false, 0, 0, false, false}; }
constexpr DebugConvRow wino(int code, ConvPath path, int tune) { return {code, path, Operand::F32, false, tune, 0, false, false}; }
constexpr DebugConvRow poly(int code, ConvPath path, bool up, bool thread_writer = false) { return {code, path, Operand::F32, false, 0, 0, up, thread_writer}; }
constexpr DebugConvRow fused(int code, ConvPath path, int variant) { return {code, path, Operand::F32, false, 0, variant, false, false}; }
constexpr DebugConvRow kDebugConv[] = {
    direct(0, Operand::F32, false, 0),
    on_path(1, ConvPath::Valu),
    wino(2, ConvPath::WinoF2, 0), wino(12, ConvPath::WinoF2, 71), wino(22, ConvPath::WinoF2, 72),
    wino(3, ConvPath::WinoF4, 0), wino(13, ConvPath::WinoF4, 71), wino(23, ConvPath::WinoF4, 72),
    poly(24, ConvPath::Poly, false), poly(25, ConvPath::Poly, true),
    poly(26, ConvPath::PolyTriples, false), poly(27, ConvPath::PolyTriples, true), poly(28, ConvPath::PolyTriples, true, true),
    on_path(48, ConvPath::F4Triples), on_path(49, ConvPath::Split3a),
    on_path(44, ConvPath::F4Pairs, Operand::F16), on_path(45, ConvPath::F4Pairs, Operand::BF16),
    on_path(46, ConvPath::DirectPair, Operand::F16), on_path(47, ConvPath::DirectPair, Operand::BF16),
    on_path(33, ConvPath::Fused32),
    fused(34, ConvPath::Fused64, 0), fused(36, ConvPath::Fused64, 64), fused(55, ConvPath::Fused64, 20),               // 64: + cout block by XCD where legal; 20: the production variant by number
    fused(35, ConvPath::Fused64Pair, 4), fused(37, ConvPath::Fused64Pair, 4 + 64), fused(56, ConvPath::Fused64Pair, 24),
    fused(62, ConvPath::Fused64T, 0), fused(63, ConvPath::Fused64T, 64),
    // 16-bit operands: production dispatch, the generic 256 / 128 tile, the 512- / 256-pixel halo kernel
    direct(4, Operand::BF16, false, 0), direct(160, Operand::BF16, false, 60), direct(161, Operand::BF16, false, 61), direct(162, Operand::BF16, false, 64),
    direct(163, Operand::BF16, false, 65),
    direct(5, Operand::F16, false, 0), direct(165, Operand::F16, false, 61), direct(166, Operand::F16, false, 64), direct(167, Operand::F16, false, 65),
    direct(204, Operand::BF16, true, 0), direct(260, Operand::BF16, true, 60), direct(261, Operand::BF16, true, 61), direct(262, Operand::BF16, true, 64),
    direct(263, Operand::BF16, true, 65),
    // 100 + a tuning code of the f32 kernels
    direct(100, Operand::F32, false, 0), direct(103, Operand::F32, false, 3), direct(105, Operand::F32, false, 5), direct(106, Operand::F32, false, 6),
    direct(107, Operand::F32, false, 7), direct(150, Operand::F32, false, 50), direct(170, Operand::F32, false, 70), direct(171, Operand::F32, false, 71),
    direct(172, Operand::F32, false, 72), direct(173, Operand::F32, false, 73),
};

enum class BenchKind {
    Conv,             // launch_conv: operand mode, PAIR kernels, bf16 activation storage, tuning code
    Fused32,          // wino_fused.hip: tuning-aid flags
    Fused32Stamps,    // once, with its phase timeline printed
    Wino3,            // the three-launch F(4x4,3x3) path on the f32 GEMM
    Wino3Gemm,        // its component GEMMs alone
    Fused64,          // launch_wino_fused64: launch variant (fp16 operands: the pair twin's weights)
    Fused64Stamps,    // once, with its per-wave cycle budget printed: stamp variant
    Fused64T,         // launch_wino_fused64t: launch variant
    Fused64TStamps,   // once, with its per-wave cycle stamps printed: stamp variant
    PairGemm,         // the pair GEMM alone: ablation twin
    TripleGemm,       // the three-piece GEMM alone: 5 launch twin + ablation twin
    Split3aGemm,      // a 1x1 layer on gemm_split3a_kernel alone: 5 launch twin + ablation twin
};
struct BenchRow {
    int lo, hi;   // the codes lo .. hi
    BenchKind kind;
    int arg;      // of code lo; code lo + i carries arg + i (bench_conv_lookup): tuning code, flags, launch / stamp / ablation variant as the kind names it
    Operand op;
    bool pair;       // Conv: the PAIR kernels on hi + lo pieces of kind `op`
    bool act_bf16;   // Conv: bf16 activation storage
};
constexpr BenchRow bench(int lo, int hi, BenchKind kind, int arg, Operand op = Operand::F32, bool pair = false, bool act_bf16 = false) {
    return {lo, hi, kind, arg, op, pair, act_bf16};
}
constexpr BenchRow kBenchConv[] = {
    bench(0, 0, BenchKind::Conv, 0), bench(3, 3, BenchKind::Conv, 3), bench(5, 7, BenchKind::Conv, 5), bench(50, 50, BenchKind::Conv, 50),
    bench(70, 73, BenchKind::Conv, 70),
    bench(60, 61, BenchKind::Conv, 60, Operand::BF16),                 // 256 / 128 tile
    bench(62, 62, BenchKind::Conv, 0, Operand::BF16),                  // automatic, incl. the halo kernel
    bench(63, 63, BenchKind::Conv, 0, Operand::BF16, false, true),
    bench(64, 65, BenchKind::Conv, 64, Operand::BF16),                 // 62 / 63 with the 512- / 256-pixel halo kernel forced
    bench(66, 67, BenchKind::Conv, 64, Operand::BF16, false, true),
    bench(480, 480, BenchKind::Conv, 0, Operand::F16, true), bench(481, 481, BenchKind::Conv, 0, Operand::BF16, true),
    bench(482, 482, BenchKind::Conv, 61, Operand::F16, true),          // 480 without the 256 x 256 tile
    bench(80, 80, BenchKind::Fused32, 0),
    bench(83, 82 + 255, BenchKind::Fused32, 1),                        // flags 1 .. 255: 1 no patch traffic, 2 no weight traffic, 4 / 8 producer / MFMA waves at s_setprio 2
    bench(82, 82, BenchKind::Fused32Stamps, 0),
    bench(81, 81, BenchKind::Wino3, 0), bench(421, 421, BenchKind::Wino3Gemm, 0),
    bench(430, 432, BenchKind::Fused64, 20),                           // r04 persistent kernel: production, weight fragments / patch loads read zeros
    bench(434, 434, BenchKind::Fused64, 24, Operand::F16),             // its fp16-pair twin
    bench(435, 435, BenchKind::Fused64Stamps, 25), bench(2004, 2004, BenchKind::Fused64Stamps, 25),
    bench(2001, 2002, BenchKind::Fused64Stamps, 28),                   // the stamp twins without weight / patch traffic
    bench(460, 462, BenchKind::Fused64T, 0),                           // r06 two-tile-group kernel: production, weight fragments / patch gathers read zeros
    bench(467, 469, BenchKind::Fused64T, 6),                           // measurement twins: no transform arithmetic / + no gathers / no gathers only
    bench(465, 465, BenchKind::Fused64TStamps, 5),
    bench(4650, 4653, BenchKind::Fused64TStamps, 12),                  // no patch traffic / output stores dropped / residual loads dropped / the coalesced-epilogue twin
    bench(472, 476, BenchKind::PairGemm, 0),                           // full, no loads, (none), no MFMAs, no output stores: launch_gemm_split_pairs refuses the one it lacks
    bench(490, 504, BenchKind::TripleGemm, 0),                         // split3_launch_twin(arg / 5, arg % 5)
    bench(510, 524, BenchKind::Split3aGemm, 0),                        // the same numbering on gemm_split3a_kernel (K = 1, stride 1, no epilogue but none)
};

template <class Row, size_t N, class Lo, class Hi>
constexpr bool codes_disjoint(const Row (&rows)[N], Lo lo, Hi hi) {
    for (size_t i = 0; i < N; ++i)
        for (size_t j = 0; j < N; ++j)
            if (i != j && lo(rows[i]) <= hi(rows[j]) && lo(rows[j]) <= hi(rows[i])) return false;
    return true;
}
constexpr int row_code(const DebugConvRow& r) { return r.code; }
constexpr int row_lo(const BenchRow& r) { return r.lo; }
constexpr int row_hi(const BenchRow& r) { return r.hi; }
static_assert(codes_disjoint(kDebugConv, row_code, row_code), "irsde_debug_conv: a selector code has two rows");
static_assert(codes_disjoint(kBenchConv, row_lo, row_hi), "irsde_bench_conv: a variant has two rows");

const DebugConvRow& debug_conv_lookup(int code) {
    for (const DebugConvRow& r : kDebugConv)
        if (r.code == code) return r;
    throw HipError("debug_conv: unknown selector code " + std::to_string(code));
}
struct BenchSel {
    const BenchRow& row;
    int arg;
};
BenchSel bench_conv_lookup(int code) {
    for (const BenchRow& r : kBenchConv)
        if (code >= r.lo && code <= r.hi) return {r, r.arg + (code - r.lo)};
    throw HipError("bench_conv: unknown variant " + std::to_string(code));
}

// The arguments of ncomp GEMMs C_z [M][N] = A_z [M][K] . B_z [N][K]^T over split operands (pA / pB: unsigned shorts resp. elements per component, as the launcher counts them)
SplitGemmArgs split_gemm_args(const unsigned short* a, const unsigned short* b, float* C, int M, int N, int K, size_t pA, size_t pB) {
    SplitGemmArgs g;
    g.a = a; g.b = b; g.out = C;
    g.pA = (long long)pA; g.pB = (long long)pB; g.pO = (long long)M * N;
    g.M = M; g.N = N; g.K = K; g.lda = K; g.ldc = N;
    return g;
}
// f32 operands [ncomp][M][K] and [ncomp][N][K] on the device -> their three-piece / pair copies in `mem` and the GEMM arguments over them
SplitGemmArgs split_triples(Scratch& mem, const float* A, const float* Bm, float* C, int M, int N, int K, int ncomp, hipStream_t s) {
    const size_t ea = split3_comp_elems((size_t)M, (size_t)K), eb = split3_comp_elems((size_t)N, (size_t)K);
    unsigned short *ta = mem.alloc<unsigned short>(ea * ncomp), *tb = mem.alloc<unsigned short>(eb * ncomp);
    launch_split_triples(A, ta, ncomp, (size_t)M, K, s);
    launch_split_triples(Bm, tb, ncomp, (size_t)N, K, s);
    return split_gemm_args(ta, tb, C, M, N, K, ea, eb);
}
// (fp16 pieces: of A * sa and B * sb, powers of two, undone by out_scale)
SplitGemmArgs split_pairs(Scratch& mem, const float* A, const float* Bm, float* C, int M, int N, int K, int ncomp, hipStream_t s, bool f16 = false, float sa = 1.f,
                          float sb = 1.f) {
    unsigned short *pa = mem.alloc<unsigned short>((size_t)2 * ncomp * M * K), *pb = mem.alloc<unsigned short>((size_t)2 * ncomp * N * K);
    launch_split_pairs(A, pa, (size_t)ncomp * M, K, s, f16, sa);
    launch_split_pairs(Bm, pb, (size_t)ncomp * N, K, s, f16, sb);
    SplitGemmArgs g = split_gemm_args(pa, pb, C, M, N, K, (size_t)M * K, (size_t)N * K);
    g.out_scale = 1.0f / (sa * sb);
    return g;
}

// The line irsde_debug_conv_choice and irsde_debug_conv_features report a ConvChoice with
void write_choice_line(const ConvChoice& c, char* out, int out_len) {
    snprintf(out, (size_t)out_len, "name=%s family=%d tile=%dx%d op=%d act=%d inscale=%d zbatch=%d zrows=%d grid=%ux%ux%u threads=%d lds=%d row=%d of %d",
             c.name().c_str(), (int)c.family, c.BM, c.BN, (int)c.op, (int)c.act, (int)c.inscale, c.zbatch, c.zrows, c.gx, c.gy, c.gz, c.threads, c.lds, c.row,
             conv_instance_count());
}

// The line irsde_debug_conv_halo_choice reports a HaloChoice with (irsde_debug_conv_features appends it to the choice line of a halo launch)
void write_halo_line(const HaloChoice& h, char* out, int out_len) {
    snprintf(out, (size_t)out_len, "kernel=halo%d bn=%d op=%d act=%d tiles=%dx%d nblk_n=%d nslow=%d grid=%u lds=%d instance=%d of %d", h.pixels, h.BN, h.op, h.act,
             h.tiles_x, h.tiles_y, h.nblk_n, h.n_slow, h.grid, h.lds, h.instance, kHaloInstances);
}

// The layer the two host-only choice hooks describe: pixel strides = channel counts, every tensor stands for "present"
ConvParams choice_hook_params(int B, int Hin, int Win, int C0, int C1, int Cout, int K, int stride, int pad, int in_shift, int operand, int storage, int pair,
                              unsigned features, int splits, int nz) {
    static const float dummy[4] = {};   // stands for every tensor: the choice reads which pointers are set, never what they point at
    float* const some = const_cast<float*>(dummy);
    auto bit = [&](int i) { return (features >> i & 1u) ? some : nullptr; };
    ConvParams p;
    p.in0 = some; p.C0 = C0; p.pix0 = C0; p.in1 = C1 ? some : nullptr; p.C1 = C1; p.pix1 = C1;
    p.Hin = Hin; p.Win = Win; p.in_shift = in_shift;
    p.w = some; p.Cout = Cout; p.KH = K; p.KW = K; p.stride = stride; p.pad_y = pad; p.pad_x = pad;
    p.B = B;
    p.Ho = ((Hin << in_shift) + 2 * pad - K) / stride + 1;
    p.Wo = ((Win << in_shift) + 2 * pad - K) / stride + 1;
    p.out = some; p.out_stride = Cout; p.res_stride = Cout; p.zeros = some;
    p.bias = bit(0); p.film = bit(1); p.silu = bit(2) != nullptr; p.res = bit(3); p.in_scale = bit(4); p.ch_scale = bit(5);
    p.gate = bit(6) != nullptr; p.shuffle = bit(7) != nullptr; p.ln_g = bit(8);
    if (pair) p.w_pair = reinterpret_cast<const unsigned short*>(some);
    else if (operand) p.w_bf = reinterpret_cast<const unsigned short*>(some);
    p.f16 = operand == 2;
    p.in_bf16 = p.out_bf16 = storage == 1;
    p.in_f16 = p.out_f16 = storage == 2;
    p.nz = nz;
    if (splits > 1) { p.splits = splits; p.partial = some; }
    return p;
}

// What irsde_debug_scam and irsde_debug_scam_full share; the projections run on the B x Hs x Ws map of each view.  In order: the argument check, the hook's own
// check_shape(), the two views' packed projection weights, the uploads and the [in2 | qv | F] scratch, the hook's prologue(dev, s), the two [LN(x) | x] -> [Q | V]
// GEMMs, the hook's tail(dev, s) = its core + epilogue
struct ScamHookArgs {   // the hooks' pointers, in their parameter order
    const float* x;
    float* out;
    const float *norm_l_g, *norm_r_g, *l_proj1_w, *l_proj1_b, *r_proj1_w, *r_proj1_b, *l_proj2_w, *l_proj2_b, *r_proj2_w, *r_proj2_b, *beta, *gamma;
};
struct ScamHookDev {
    float *gl, *gr, *beta, *gamma;   // device copies of norm_l.g / norm_r.g / beta / gamma
    float *in2, *qv, *F;
    size_t vsz;                      // one view's [LN(x) | x] / [Q | V]: B Hs Ws 2C floats
};
template <class ShapeCheck, class Prologue, class Tail>
void scam_hook(const ScamHookArgs& a, int B, int Hs, int Ws, int C, void* stream, ShapeCheck check_shape, Prologue prologue, Tail tail) {
    if (!a.x || !a.out || !a.norm_l_g || !a.norm_r_g || !a.l_proj1_w || !a.l_proj1_b || !a.r_proj1_w || !a.r_proj1_b || !a.l_proj2_w || !a.l_proj2_b ||
        !a.r_proj2_w || !a.r_proj2_b || !a.beta || !a.gamma)
        throw HipError("null argument");
    check_shape();
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    conv_global_init();
    std::vector<float> wl, bl, wr, br;
    scam_pack_proj(a.l_proj1_w, a.l_proj1_b, a.l_proj2_w, a.l_proj2_b, C, wl, bl);
    scam_pack_proj(a.r_proj1_w, a.r_proj1_b, a.r_proj2_w, a.r_proj2_b, C, wr, br);
    Scratch mem(s);
    auto up = [&](const float* h, size_t n) {
        float* d = mem.alloc<float>(std::max<size_t>(n, 16));
        if (h) IRSDE_HIP_CHECK(hipMemcpy(d, h, n * 4, hipMemcpyHostToDevice));
        return d;
    };
    ScamHookDev d;
    d.gl = up(a.norm_l_g, C); d.gr = up(a.norm_r_g, C); d.beta = up(a.beta, C); d.gamma = up(a.gamma, C);
    float *dwl = up(wl.data(), wl.size()), *dbl = up(bl.data(), bl.size()), *dwr = up(wr.data(), wr.size()), *dbr = up(br.data(), br.size());
    d.vsz = (size_t)B * Hs * Ws * 2 * C;
    d.in2 = up(nullptr, 2 * d.vsz); d.qv = up(nullptr, 2 * d.vsz); d.F = up(nullptr, d.vsz);
    float* dz = up(nullptr, 256);
    IRSDE_HIP_CHECK(hipMemset(dz, 0, 1024));
    prologue(d, s);
    for (int v = 0; v < 2; ++v) {
        ConvParams p;
        p.in0 = d.in2 + v * d.vsz; p.C0 = 2 * C; p.pix0 = 2 * C;
        p.Hin = Hs; p.Win = Ws;
        p.w = v ? dwr : dwl; p.Cout = 2 * C; p.KH = p.KW = 1; p.stride = 1;
        p.B = B; p.Ho = Hs; p.Wo = Ws;
        p.out = d.qv + v * d.vsz; p.out_stride = 2 * C;
        p.bias = v ? dbr : dbl;
        p.zeros = dz;
        launch_conv(p, s);
    }
    tail(d, s);
    IRSDE_HIP_CHECK(hipStreamSynchronize(s));
}

// the hooks' common shape check: what a network level can produce (N a multiple of 4) inside the grids of the kernels (4 B blocks in y)
void attn_hook_shape(const char* who, int B, int N) {
    if (B < 1 || B > 16383 || N < 4 || N % 4) throw HipError(std::string(who) + ": B in [1, 16383], N a positive multiple of 4");
}
// Builder::attn_workspace on hook scratch, every float NaN: a partial a kernel does not write shows in the result
AttnWorkspace attn_hook_workspace(Scratch& mem, int B, int N, hipStream_t s) {
    AttnWorkspace ws;
    ws.nch = attn_num_chunks(N, B);
    const size_t n[4] = {(size_t)B * ws.nch * 128, (size_t)B * 4 * ws.nch * 1024, (size_t)B * 4 * ws.nch * 32, (size_t)B * 4 * 1024};
    float** const dst[4] = {&ws.pmax, &ws.pctx, &ws.psum, &ws.ctx};
    for (int i = 0; i < 4; ++i) {
        *dst[i] = mem.alloc<float>(n[i]);
        IRSDE_HIP_CHECK(hipMemsetAsync(*dst[i], 0xFF, n[i] * sizeof(float), s));
    }
    return ws;
}

}  // namespace
}  // namespace irsde

extern "C" {

int irsde_debug_scam(const float* x, int B, int H, int W, int C, const float* norm_l_g, const float* norm_r_g, const float* l_proj1_w,
                     const float* l_proj1_b, const float* r_proj1_w, const float* r_proj1_b, const float* l_proj2_w, const float* l_proj2_b,
                     const float* r_proj2_w, const float* r_proj2_b, const float* beta, const float* gamma, float* out, void* stream) {
    return guard([&] {
        scam_hook(
            {x, out, norm_l_g, norm_r_g, l_proj1_w, l_proj1_b, r_proj1_w, r_proj1_b, l_proj2_w, l_proj2_b, r_proj2_w, r_proj2_b, beta, gamma}, B, H / 4, W / 4, C, stream,
            [&] {
                if (B < 1) throw HipError("debug_scam: bad shape");
                scam_check_shape(H, W, C);
            },
            [&](const ScamHookDev& d, hipStream_t s) { launch_scam_prologue(x, d.gl, d.gr, d.in2, B, H, W, C, s); },
            [&](const ScamHookDev& d, hipStream_t s) {
                launch_scam_core(d.qv, d.F, B, H, W, C, s);
                launch_scam_epilogue(x, d.F, d.beta, d.gamma, out, B, H, W, C, s);
            });
    });
}

int irsde_debug_scam_full(const float* x, int B, int H, int W, int C, const float* norm_l_g, const float* norm_r_g, const float* l_proj1_w,
                          const float* l_proj1_b, const float* r_proj1_w, const float* r_proj1_b, const float* l_proj2_w, const float* l_proj2_b,
                          const float* r_proj2_w, const float* r_proj2_b, const float* beta, const float* gamma, float* out, void* stream) {
    return guard([&] {
        scam_hook(
            {x, out, norm_l_g, norm_r_g, l_proj1_w, l_proj1_b, r_proj1_w, r_proj1_b, l_proj2_w, l_proj2_b, r_proj2_w, r_proj2_b, beta, gamma}, B, H, W, C, stream,
            [&] {
                if (B < 1 || (long long)B * H > 65535) throw HipError("debug_scam_full: bad shape");
                scam_full_check_shape(H, W, C);
            },
            [&](const ScamHookDev& d, hipStream_t s) { launch_scam_full_prologue(x, d.gl, d.gr, d.in2, B, H, W, C, s); },
            [&](const ScamHookDev& d, hipStream_t s) {
                launch_scam_full_core(d.qv, d.F, B, H, W, C, s);
                if (out != x) IRSDE_HIP_CHECK(hipMemcpyAsync(out, x, d.vsz * sizeof(float), hipMemcpyDeviceToDevice, s));   // (vsz = 2 B H W C: the whole tensor)
                launch_scam_full_epilogue(out, d.F, d.beta, d.gamma, B, H, W, C, s);
            });
    });
}

int irsde_debug_scam_stream(const float* x, int B, int H, int W, int C, const float* norm_l_g, const float* norm_r_g, const float* l_proj1_w,
                            const float* l_proj1_b, const float* r_proj1_w, const float* r_proj1_b, const float* l_proj2_w, const float* l_proj2_b,
                            const float* r_proj2_w, const float* r_proj2_b, const float* beta, const float* gamma, int block_w, float* out, void* stream) {
    return guard([&] {
        scam_hook(
            {x, out, norm_l_g, norm_r_g, l_proj1_w, l_proj1_b, r_proj1_w, r_proj1_b, l_proj2_w, l_proj2_b, r_proj2_w, r_proj2_b, beta, gamma}, B, H / 4, W / 4, C, stream,
            [&] {
                if (B < 1 || (long long)B * (H / 4) > 65535) throw HipError("debug_scam_stream: bad shape");
                if (block_w != 0 && !scam_stream_block_ok(block_w)) throw HipError("debug_scam_stream: block_w must be 0 or a multiple of 16 in [16, 512]");
                scam_check_shape(H, W, C, true);
            },
            [&](const ScamHookDev& d, hipStream_t s) { launch_scam_prologue(x, d.gl, d.gr, d.in2, B, H, W, C, s); },
            [&](const ScamHookDev& d, hipStream_t s) {
                launch_scam_stream_core(d.qv, d.F, B, H / 4, W / 4, C, block_w, s);
                launch_scam_epilogue(x, d.F, d.beta, d.gamma, out, B, H, W, C, s);
            });
    });
}

int irsde_debug_scam_full_stream(const float* x, int B, int H, int W, int C, const float* norm_l_g, const float* norm_r_g, const float* l_proj1_w,
                                 const float* l_proj1_b, const float* r_proj1_w, const float* r_proj1_b, const float* l_proj2_w, const float* l_proj2_b,
                                 const float* r_proj2_w, const float* r_proj2_b, const float* beta, const float* gamma, int block_w, float* out,
                                 void* stream) {
    return guard([&] {
        scam_hook(
            {x, out, norm_l_g, norm_r_g, l_proj1_w, l_proj1_b, r_proj1_w, r_proj1_b, l_proj2_w, l_proj2_b, r_proj2_w, r_proj2_b, beta, gamma}, B, H, W, C, stream,
            [&] {
                if (B < 1 || (long long)B * H > 65535) throw HipError("debug_scam_full_stream: bad shape");
                if (block_w != 0 && !scam_stream_block_ok(block_w)) throw HipError("debug_scam_full_stream: block_w must be 0 or a multiple of 16 in [16, 512]");
                scam_full_check_shape(H, W, C, true);
            },
            [&](const ScamHookDev& d, hipStream_t s) { launch_scam_full_prologue(x, d.gl, d.gr, d.in2, B, H, W, C, s); },
            [&](const ScamHookDev& d, hipStream_t s) {
                launch_scam_stream_core(d.qv, d.F, B, H, W, C, block_w, s);
                if (out != x) IRSDE_HIP_CHECK(hipMemcpyAsync(out, x, d.vsz * sizeof(float), hipMemcpyDeviceToDevice, s));   // (vsz = 2 B H W C: the whole tensor)
                launch_scam_full_epilogue(out, d.F, d.beta, d.gamma, B, H, W, C, s);
            });
    });
}

int irsde_debug_force_scam_stream(int block_w) {
    if (block_w != 0 && !scam_stream_block_ok(block_w)) return guard([&] { throw HipError("debug_force_scam_stream: block_w must be 0 or a multiple of 16 in [16, 512]"); });
    set_force_scam_stream(block_w);
    return IRSDE_OK;
}

int irsde_debug_naf_gate_sca(const float* u, int B, int H, int W, int c, const float* conv2_w, const float* conv2_b, const float* sca_w, const float* sca_b,
                             float* gated_out, float* mean_out, float* s_out, void* stream) {
    return guard([&] {
        if (!u || !conv2_w || !conv2_b || !sca_w || !sca_b || !gated_out || !s_out) throw HipError("null argument");
        if (B < 1 || B > 65535 || H < 1 || W < 1 || c < 4 || c % 4 || (long long)H * W >= (1ll << 31)) throw HipError("debug_naf_gate_sca: bad shape");
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        conv_global_init();
        Scratch mem(s);
        float *dw = mem.upload(pack_dwconv_taps(conv2_w, 2 * c)), *db = mem.upload(conv2_b, (size_t)2 * c);
        float *dsw = mem.upload(sca_w, (size_t)c * c), *dsb = mem.upload(sca_b, c);
        const int nt = dwgate_tiles(H, W, c);
        float *partial = mem.alloc<float>((size_t)B * nt * c), *mean = mem.alloc<float>((size_t)B * c);
        launch_dwconv_gate(u, dw, db, gated_out, partial, B, H, W, c, s);
        launch_sca(partial, nt, dsw, dsb, mean, s_out, B, c, H * W, s);
        if (mean_out) launch_sca_mean(partial, nt, mean_out, B, c, H * W, s);   // (the one-launch route keeps its mean in LDS: the same sums from the same partials)
        IRSDE_HIP_CHECK(hipStreamSynchronize(s));
    });
}

int irsde_debug_tlsc(const float* g, int B, int h, int w, int c, int k1, int k2, float* pooled_out, const float* scale_map, float* scaled_out, void* stream) {
    return guard([&] {
        if (!g || !pooled_out || !scale_map || !scaled_out) throw HipError("null argument");
        tlsc_check_shape(B, h, w, c, k1, k2);
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        conv_global_init();
        Scratch mem(s);
        float* rowsum = mem.alloc<float>((size_t)B * h * (w - k2 + 1) * c);
        launch_tlsc_pool(g, rowsum, pooled_out, B, h, w, c, k1, k2, s);
        IRSDE_HIP_CHECK(hipMemcpyAsync(scaled_out, g, (size_t)B * h * w * c * sizeof(float), hipMemcpyDeviceToDevice, s));
        launch_tlsc_scale(scaled_out, scale_map, B, h, w, c, k1, k2, s);
        IRSDE_HIP_CHECK(hipStreamSynchronize(s));
    });
}

int irsde_debug_ln_film(const float* x, long long M, int C, long long ppi, const float* g, const float* fscale, const float* fshift, int film_bstride,
                        float* out, void* stream) {
    return guard([&] {
        if (!x || !g || !fscale || !fshift || !out) throw HipError("null argument");
        if (M < 1 || ppi < 1 || C < 4 || C % 4 || C > 2048 || film_bstride < 0 || film_bstride % 4) throw HipError("debug_ln_film: bad shape");
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        conv_global_init();
        Scratch mem(s);
        float* dg = mem.upload(g, C);
        launch_layernorm_film(x, dg, fscale, fshift, film_bstride, ppi, out, M, C, 1e-5f, s);
        IRSDE_HIP_CHECK(hipStreamSynchronize(s));
    });
}

int irsde_debug_full_attention16(const void* qkv_bf16, int B, int N, void* out_bf16, void* stream) {
    return guard([&] {
        if (!qkv_bf16 || !out_bf16) throw HipError("null argument");
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        launch_full_attention16(static_cast<const unsigned short*>(qkv_bf16), static_cast<unsigned short*>(out_bf16), B, N, s);
        IRSDE_HIP_CHECK(hipStreamSynchronize(s));
    });
}

int irsde_debug_attn_choice(int C, int mode, int act_bf16, int N, int B, char* out, int out_len) {
    return guard([&] {
        if (!out || out_len < 1 || mode < 0 || mode > 4 || N < 1 || B < 1) throw HipError("debug_attn_choice: bad argument");
        const AttnChoice c = attn_choice(C, static_cast<AttnMode>(mode), act_bf16 != 0, N, B);
        snprintf(out, (size_t)out_len, "kv_row=%d of %d qo_row=%d of %d kv_lds=%zu qo_lds=%zu kv_tile=%d qo_tile=%d chunk_len=%d nch=%d", c.kv_row, c.kv_rows,
                 c.qo_row, c.qo_rows, c.kv_lds, c.qo_lds, c.kv_tile, c.qo_tile, c.chunk_len, c.nch);
    });
}

int irsde_debug_attn_block(const float* x, int B, int N, int C, const float* norm_g, const float* to_qkv_w, const float* to_out_w, const float* to_out_b,
                           const float* to_out_g, int mode, int act_bf16, float* y, void* stream) {
    return guard([&] {
        if (!x || !norm_g || !to_qkv_w || !to_out_w || !to_out_b || !to_out_g || !y) throw HipError("null argument");
        if (mode < 0 || mode > 4) throw HipError("debug_attn_block: mode must be 0 .. 4 (AttnMode)");
        attn_hook_shape("debug_attn_block", B, N);
        AttnProj p;
        p.mode = static_cast<AttnMode>(mode);
        p.act_bf16 = act_bf16 != 0;
        attn_require_instance(false, C, p.mode, p.act_bf16);   // every refusal of the two launchers before the first launch
        attn_require_instance(true, C, p.mode, p.act_bf16);
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        conv_global_init();
        Scratch mem(s);
        const size_t nq = (size_t)128 * C, nkv = (size_t)256 * C, no = (size_t)C * 128, nx = (size_t)B * N * C;
        float *dqkv = mem.upload(to_qkv_w, nq + nkv), *dwo = mem.upload(to_out_w, no), *dbo = mem.upload(to_out_b, C);
        float *g1 = mem.upload(norm_g, C), *g2 = mem.upload(to_out_g, C);
        const float *wq = dqkv, *wkv = dqkv + nq;
        // the planes of the mode, by the functions behind the engine's bf16_copy / pair_copy / triple_copy (Builder::attn_proj)
        if (p.mode == AttnMode::Bf16 || p.mode == AttnMode::Fp16) {
            unsigned short *q16 = mem.alloc<unsigned short>(nq + nkv), *o16 = mem.alloc<unsigned short>(no);
            if (p.mode == AttnMode::Fp16) { launch_f32_to_f16(dqkv, q16, nq + nkv, s); launch_f32_to_f16(dwo, o16, no, s); }
            else { launch_f32_to_bf16(dqkv, q16, nq + nkv, s); launch_f32_to_bf16(dwo, o16, no, s); }
            p.q = q16; p.kv = q16 + nq; p.out = o16;
        } else if (p.mode == AttnMode::Bf16x3) {
            unsigned short *kv3 = mem.alloc<unsigned short>(3 * nkv), *q3 = mem.alloc<unsigned short>(3 * nq), *o3 = mem.alloc<unsigned short>(3 * no);
            launch_split_frag3(wkv, kv3, 256, C, s);
            launch_split_frag3(wq, q3, 128, C, s);
            launch_split_frag3(dwo, o3, (size_t)C, 128, s);
            p.kv = kv3; p.q = q3; p.out = o3;
        } else if (p.mode == AttnMode::PairF16) {
            auto pair = [&](const float* host, const float* dev, size_t n, float& inv) {
                const float sc = pow2_scale_into_512(host, n);
                unsigned short* d = mem.alloc<unsigned short>(2 * n);
                launch_split_planes(dev, d, n, n, 2, s, true, sc);
                inv = 1.0f / sc;
                return d;
            };
            p.kv = pair(to_qkv_w + nq, wkv, nkv, p.kv_inv);
            p.q = pair(to_qkv_w, wq, nq, p.q_inv);
            p.out = pair(to_out_w, dwo, no, p.out_inv);
        }
        const AttnWorkspace ws = attn_hook_workspace(mem, B, N, s);
        const float* xin = x;
        float* yout = y;
        unsigned short* y16 = nullptr;
        if (p.act_bf16) {   // the caller's fp32 x rounded into a bf16 copy; the bf16 result starts as NaN and is widened back
            unsigned short* x16 = mem.alloc<unsigned short>(nx);
            y16 = mem.alloc<unsigned short>(nx);
            launch_f32_to_bf16(x, x16, nx, s);
            IRSDE_HIP_CHECK(hipMemsetAsync(y16, 0xFF, nx * 2, s));
            xin = reinterpret_cast<const float*>(x16);
            yout = reinterpret_cast<float*>(y16);
        }
        launch_attention_kv_context(xin, wkv, B, N, C, ws, s, g1, 1e-5f, p);
        launch_attention_q_out_fused(xin, xin, wq, dwo, dbo, g2, yout, B, N, C, 1e-5f, ws, s, g1, p);
        if (y16) launch_bf16_to_f32(y16, y, nx, s);
        IRSDE_HIP_CHECK(hipStreamSynchronize(s));
    });
}

int irsde_debug_attn_core(int route, const float* in, int B, int N, int C, const float* wkv, const float* q, int bf16, float* out, void* stream) {
    return guard([&] {
        if (route != 1 && route != 2) throw HipError("debug_attn_core: route must be 1 (k / v context from xn + q tensor) or 2 (q | k | v tensor)");
        if (!in || !out || (route == 1 && (!wkv || !q))) throw HipError("null argument");
        attn_hook_shape("debug_attn_core", B, N);
        if (route == 1 && bf16) throw HipError("debug_attn_core: route 1 runs on fp32 tensors only");
        if (route == 1) attn_require_instance(false, C, AttnMode::F32, false);
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        conv_global_init();
        Scratch mem(s);
        const AttnWorkspace ws = attn_hook_workspace(mem, B, N, s);
        if (route == 1) {
            const float* dwkv = mem.upload(wkv, (size_t)256 * C);
            launch_attention_kv_context(in, dwkv, B, N, C, ws, s);
            launch_attention_q_out(q, out, B, N, ws, s);
        } else if (bf16) {
            const size_t ni = (size_t)B * N * 384, no = (size_t)B * N * 128;
            unsigned short *i16 = mem.alloc<unsigned short>(ni), *o16 = mem.alloc<unsigned short>(no);
            launch_f32_to_bf16(in, i16, ni, s);
            IRSDE_HIP_CHECK(hipMemsetAsync(o16, 0xFF, no * 2, s));
            launch_linear_attention(reinterpret_cast<const float*>(i16), reinterpret_cast<float*>(o16), B, N, ws, s, true);
            launch_bf16_to_f32(o16, out, no, s);
        } else {
            launch_linear_attention(in, out, B, N, ws, s, false);
        }
        IRSDE_HIP_CHECK(hipStreamSynchronize(s));
    });
}

int irsde_debug_naf_lnconv(int mode, const float* x, long long M, int c, int Cout, long long ppi, const float* g, const float* fscale, const float* fshift,
                           int film_bstride, const float* w, const float* bias, const float* gate_film, int gate_film_bstride, const float* in_scale,
                           const float* ch_scale, const float* res, float* out, void* stream) {
    return guard([&] {
        if (mode < 0 || mode > 3) throw HipError("debug_naf_lnconv: mode must be 0 .. 3");
        if (!x || !w || !bias || !out) throw HipError("null argument");
        if (!naf_lnconv_ok(c, Cout, M) || ppi < 1) throw HipError("debug_naf_lnconv: bad shape");
        const bool ln = mode <= 1;
        if (ln && (!g || !fscale || !fshift || film_bstride < 0 || film_bstride % 4)) throw HipError("debug_naf_lnconv: modes 0 / 1 need g and the FiLM rows");
        if (mode == 1 && gate_film && gate_film_bstride < 0) throw HipError("debug_naf_lnconv: bad lens FiLM stride");
        if (!ln && (!ch_scale || !res || (mode == 2 && !in_scale))) throw HipError("debug_naf_lnconv: modes 2 / 3 need ch_scale and res, mode 2 in_scale");
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        conv_global_init();
        std::vector<float> pw, pb;
        pack_conv_rows(w, bias, Cout, c, 1, 1, mode == 1 ? naf_gate_perm(Cout / 2) : std::vector<int>(), pw, pb);
        Scratch mem(s);
        float *dwf = mem.upload(pw), *dbias = mem.upload(pb);
        unsigned short* w16 = mem.alloc<unsigned short>(pw.size());
        launch_f32_to_f16(dwf, w16, pw.size(), s);
        if (ln) {
            float* dg = mem.upload(g, c);
            launch_naf_lnconv(x, dg, fscale, fshift, film_bstride, ppi, w16, dbias, out, M, c, Cout, mode, mode == 1 ? gate_film : nullptr,
                              mode == 1 && gate_film ? gate_film_bstride : 0, s);
        } else {
            float* dcs = mem.upload(ch_scale, Cout);
            launch_naf_pwconv(x, mode == 2 ? in_scale : nullptr, ppi, w16, dbias, dcs, res, out, M, c, Cout, s);
        }
        IRSDE_HIP_CHECK(hipStreamSynchronize(s));
    });
}

int irsde_debug_naf_chain(const float* x, float* out, int B, int nblocks, const float* norm1_g, const float* conv1_w, const float* conv1_b, const float* conv2_w,
                          const float* conv2_b, const float* sca_w, const float* sca_b, const float* conv3_w, const float* conv3_b, const float* beta,
                          const float* norm2_g, const float* conv4_w, const float* conv4_b, const float* conv5_w, const float* conv5_b, const float* gamma,
                          const float* film, int film_bstride, int film_off, const float* cam, int cam_bstride, int cam_off, int groups, void* stream) {
    return guard([&] {
        if (!x || !out || !norm1_g || !conv1_w || !conv1_b || !conv2_w || !conv2_b || !sca_w || !sca_b || !conv3_w || !conv3_b || !beta || !norm2_g || !conv4_w ||
            !conv4_b || !conv5_w || !conv5_b || !gamma || !film)
            throw HipError("null argument");
        // refused before anything is launched: what a launcher cannot run (the kernel reads its rows as aligned float4)
        if (B < 1 || B > 65535 || nblocks < 1 || nblocks > 64) throw HipError("debug_naf_chain: bad B or nblocks");
        if (groups != 1 && groups != 2 && groups != 4) throw HipError("debug_naf_chain: groups must be 1, 2 or 4");
        if (film_bstride < 0 || film_bstride % 4 || film_off < 0 || film_off % 4) throw HipError("debug_naf_chain: bad FiLM stride / offset");
        if (cam && (cam_bstride < 0 || cam_bstride % 4 || cam_off < 0 || cam_off % 4)) throw HipError("debug_naf_chain: bad lens FiLM stride / offset");
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        conv_global_init();
        if (groups > 1 && naf_chain_split_groups(B, groups) > device_cu_count())
            throw HipError("debug_naf_chain: more work-groups than compute units (they must be co-resident)");
        constexpr size_t C = 512;
        std::vector<NafChainHostW> blocks(nblocks);
        for (int i = 0; i < nblocks; ++i) {
            NafChainHostW& b = blocks[i];
            const size_t k = (size_t)i;
            b.norm1_g = norm1_g + k * C; b.conv1_w = conv1_w + k * 2 * C * C; b.conv1_b = conv1_b + k * 2 * C;
            b.conv2_w = conv2_w + k * 18 * C; b.conv2_b = conv2_b + k * 2 * C;
            b.sca_w = sca_w + k * C * C; b.sca_b = sca_b + k * C;
            b.conv3_w = conv3_w + k * C * C; b.conv3_b = conv3_b + k * C; b.beta = beta + k * C;
            b.norm2_g = norm2_g + k * C; b.conv4_w = conv4_w + k * 2 * C * C; b.conv4_b = conv4_b + k * 2 * C;
            b.conv5_w = conv5_w + k * C * C; b.conv5_b = conv5_b + k * C; b.gamma = gamma + k * C;
        }
        std::vector<unsigned short> w;
        std::vector<float> vecs;
        pack_naf_chain_host(blocks, w, vecs);
        Scratch mem(s);
        unsigned short* dw = mem.alloc<unsigned short>(w.size());
        IRSDE_HIP_CHECK(hipMemcpy(dw, w.data(), w.size() * 2, hipMemcpyHostToDevice));
        float* dvec = mem.upload(vecs);
        if (groups == 1) {
            launch_naf_chain(x, out, dw, dvec, nblocks, B, film, film_bstride, film_off, cam, cam ? cam_bstride : 0, cam ? cam_off : 0, s, 0);
            IRSDE_HIP_CHECK(hipStreamSynchronize(s));
            return;
        }
        unsigned short* dwg = mem.alloc<unsigned short>(w.size());
        naf_chain_build_split_weights(dw, dwg, nblocks, groups, s);
        const size_t sb = naf_chain_split_scratch_bytes(B);
        char* dscratch = mem.alloc<char>(sb);
        IRSDE_HIP_CHECK(hipMemset(dscratch, 0, sb));
        launch_naf_chain_split(x, out, dwg, dvec, nblocks, B, film, film_bstride, film_off, cam, cam ? cam_bstride : 0, cam ? cam_off : 0, groups, dscratch, s);
        IRSDE_HIP_CHECK(hipStreamSynchronize(s));
        // one launch, no retry: the error word, then the barrier counters, which the kernel must leave as it found them ([B][4] in front of the error word)
        std::vector<unsigned> state((size_t)4 * B + 1);
        IRSDE_HIP_CHECK(hipMemcpy(state.data(), naf_chain_split_error_flag(dscratch, B) - 4 * B, state.size() * 4, hipMemcpyDeviceToHost));
        if (state[(size_t)4 * B]) throw HipError("debug_naf_chain: the split kernel's groups were not co-resident (spin timeout)");
        for (size_t i = 0; i < (size_t)4 * B; ++i)
            if (state[i]) throw HipError("debug_naf_chain: the split kernel left a barrier counter non-zero");
    });
}

int irsde_debug_naf_chain_split_order(int nblocks, int groups, int* order_out, long long n) {
    return guard([&] {
        if (!order_out || nblocks < 1 || nblocks > 64) throw HipError("debug_naf_chain_split_order: bad argument");
        const std::vector<int> order = naf_chain_split_order(nblocks, groups);   // (host only; refuses groups other than 2 / 4)
        if ((long long)order.size() != n) throw HipError("debug_naf_chain_split_order: the order has " + std::to_string(order.size()) + " entries");
        std::copy(order.begin(), order.end(), order_out);
    });
}

int irsde_debug_conv(const float* in0, int C0, const float* in1, int C1, int B, int Hin, int Win, int in_shift,
                     const float* w_oihw, int Cout, int KH, int KW, int stride, int pad, const float* bias,
                     const float* film, int film_bstride, int silu, const float* res, float* out, int naive,
                     int splits, void* stream) {
    return guard([&] {
        if (!in0 || !w_oihw || !out) throw HipError("null argument");
        const DebugConvRow& r = debug_conv_lookup(naive);
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        conv_global_init();
        const int Cin = C0 + C1;
        std::vector<float> pk((size_t)Cout * KH * KW * Cin);
        for (int o = 0; o < Cout; ++o)
            for (int i = 0; i < Cin; ++i)
                for (int ky = 0; ky < KH; ++ky)
                    for (int kx = 0; kx < KW; ++kx)
                        pk[(((size_t)o * KH + ky) * KW + kx) * Cin + i] = w_oihw[(((size_t)o * Cin + i) * KH + ky) * KW + kx];
        Scratch mem(s);
        float* dw = mem.upload(pk);
        float* db = bias ? mem.upload(bias, Cout) : nullptr;
        ConvParams p;
        p.in0 = in0; p.C0 = C0; p.pix0 = C0; p.in1 = in1; p.C1 = C1; p.pix1 = C1;
        p.Hin = Hin; p.Win = Win; p.in_shift = in_shift;
        p.w = dw; p.Cout = Cout; p.KH = KH; p.KW = KW; p.stride = stride; p.pad_y = pad; p.pad_x = pad;
        p.B = B;
        p.Ho = ((Hin << in_shift) + 2 * pad - KH) / stride + 1;
        p.Wo = ((Win << in_shift) + 2 * pad - KW) / stride + 1;
        p.out = out; p.out_stride = Cout; p.bias = db; p.film = film; p.film_bstride = film_bstride; p.silu = silu;
        p.res = res; p.res_stride = Cout;
        float* dz = mem.alloc<float>(256);
        IRSDE_HIP_CHECK(hipMemset(dz, 0, 1024));
        p.zeros = dz;
        if (splits > 1 && r.path != ConvPath::Valu && r.path != ConvPath::WinoF2 && r.path != ConvPath::WinoF4) {
            p.splits = splits;
            p.partial = mem.alloc<float>((size_t)splits * B * p.Ho * p.Wo * Cout);
        }
        // the three-launch and fused Winograd paths: the host weight transform U [(tile + 2)^2][Cout][Cin], the tile count, the component products M
        auto wino_weights = [&](int tile) {
            std::vector<float> U((size_t)(tile + 2) * (tile + 2) * Cout * Cin);
            wino_transform_weights(pk.data(), Cout, Cin, U.data(), tile);
            return U;
        };
        auto wino_tiles = [&](int tile) { return (long long)B * (p.Ho / tile) * (p.Wo / tile); };
        auto alloc_M = [&](int ncomp, long long T) { return mem.alloc<float>((size_t)ncomp * T * Cout); };
        // the polyphase paths: shape check, U (25 x Cout x 4 Cin resp. 100 x Cout x Cin) on the device, the plan without its V / M buffers
        auto poly_plan = [&](const char* refusal, float*& dU) {
            if (!(r.up ? wino_poly_up_shape(p) : wino_poly_down_shape(p)) || !wino_poly_eligible(p) || splits > 1) throw HipError(refusal);
            std::vector<float> U((size_t)100 * Cout * Cin);
            wino_poly_transform_weights(pk.data(), Cout, Cin, U.data(), r.up);
            dU = mem.upload(U);
            return make_wino_poly(p, dU, nullptr, nullptr);
        };
        switch (r.path) {
        case ConvPath::PolyTriples: {
            float* dU = nullptr;
            WinoPolyPlan wp = poly_plan("debug_conv: selectors 26 / 27 / 28 run what 24 / 25 run (single source, channels a multiple of 32, bias only)", dU);
            if (!gemm_split_triples_fits(wp.T, Cout, wp.K, Cout)) throw HipError("debug_conv: shape not eligible for the three-piece GEMM");
            unsigned short* dUt = mem.alloc<unsigned short>((size_t)wp.ncomp * split3_comp_elems((size_t)Cout, (size_t)wp.K));
            unsigned short* dVt = mem.alloc<unsigned short>((size_t)wp.ncomp * split3_comp_elems((size_t)wp.T, (size_t)wp.K));
            float* dM = alloc_M(wp.ncomp, wp.T);
            launch_split_triples(dU, dUt, wp.ncomp, (size_t)Cout, wp.K, s);
            wp = make_wino_poly(p, dU, nullptr, dM);
            const SplitGemmArgs sg = make_wino_poly_triples(wp, Cout, dUt, dVt, dM);
            wp.in.thread_writer = r.thread_writer;
            launch_wino_poly_input(wp.in, s);
            launch_gemm_split_triples(sg, wp.ncomp, s);
            launch_wino_poly_output(wp.out, s);
            break;
        }
        case ConvPath::Poly: {
            float* dU = nullptr;
            WinoPolyPlan wp = poly_plan(r.up ? "debug_conv: selector 25 runs a 3x3 stride-1 pad-1 convolution with in_shift = 1 (single source, channels a multiple of 32, bias only)"
                                             : "debug_conv: selector 24 runs a 4x4 stride-2 pad-1 convolution (single source, channels a multiple of 32, bias only)", dU);
            float* dV = mem.alloc<float>((size_t)wp.ncomp * wp.T * wp.K);
            wp = make_wino_poly(p, dU, dV, alloc_M(wp.ncomp, wp.T));
            launch_wino_poly_input(wp.in, s);
            launch_conv(wp.gemm, s);
            launch_wino_poly_output(wp.out, s);
            break;
        }
        case ConvPath::F4Triples: {
            if (!wino_shape_ok(p, 4) || Cin % 32) throw HipError("debug_conv: shape not eligible for the three-piece GEMM");
            const std::vector<float> U = wino_weights(4);
            const long long T = wino_tiles(4);
            if (!gemm_split_triples_fits(T, Cout, Cin, Cout)) throw HipError("debug_conv: shape not eligible for the three-piece GEMM");
            float* dU = mem.upload(U);
            unsigned short* dUt = mem.alloc<unsigned short>((size_t)36 * split3_comp_elems((size_t)Cout, (size_t)Cin));
            unsigned short* dVt = mem.alloc<unsigned short>((size_t)36 * split3_comp_elems((size_t)T, (size_t)Cin));
            launch_split_triples(dU, dUt, 36, (size_t)Cout, Cin, s);
            const WinoSplitPlan sp = make_wino_triples(p, dUt, dVt, alloc_M(36, T));
            launch_wino_input(sp.in, s);
            launch_gemm_split_triples(sp.gemm, 36, s);
            launch_wino_output(sp.out, s);
            break;
        }
        case ConvPath::Split3a: {
            if (splits > 1) p.splits = splits;
            const Split3x1Choice c = split3_1x1_choose(p, true, 2, 2, device_cu_count());
            if (!c.adopt) throw HipError(std::string("debug_conv: selector 49 runs a plain 1x1 layer (bias only): ") + c.why_not);
            unsigned short* dwt = mem.alloc<unsigned short>(split3_comp_elems((size_t)Cout, (size_t)Cin));
            launch_split_triples(dw, dwt, 1, (size_t)Cout, Cin, s);
            launch_gemm_split3a(split3_1x1_args(p, dwt), s);
            break;
        }
        case ConvPath::F4Pairs: {
            const bool f16 = r.op == Operand::F16;
            if (!wino_shape_ok(p, 4) || Cin % 32) throw HipError("debug_conv: shape not eligible for the pair GEMM");
            std::vector<float> U = wino_weights(4);
            const float us = f16 ? pow2_scale_into_512(U.data(), U.size()) : 1.f;
            const long long T = wino_tiles(4);
            float* dU = mem.upload(U);
            unsigned short* dUp = mem.alloc<unsigned short>(2 * U.size());
            unsigned short* dVp = mem.alloc<unsigned short>((size_t)36 * T * Cin * 2);
            launch_split_pairs(dU, dUp, (size_t)36 * Cout, Cin, s, f16, us);
            const WinoSplitPlan sp = make_wino_pairs(p, dUp, dVp, alloc_M(36, T), f16, us);
            launch_wino_input(sp.in, s);
            launch_gemm_split_pairs(sp.gemm, 36, s, 0, f16);
            launch_wino_output(sp.out, s);
            break;
        }
        case ConvPath::Fused64Pair: {   // the 64-cout fused kernel on fp16 hi + lo operand pairs (IRSDE_FLAG_SPLIT_F16X2's big-feature-map path)
            if (!wino_fused64_eligible(p)) throw HipError("debug_conv: shape not eligible for the fused Winograd kernel");
            std::vector<float> U = wino_weights(4), Uf(U.size());
            wino_fused64_pack_weights(U.data(), Cout, Cin, Uf.data());
            const float usc = pow2_scale_into_512(U.data(), U.size());
            float* dUf = mem.upload(Uf);
            unsigned short* dUp = mem.alloc<unsigned short>(2 * Uf.size());
            launch_wino_fused64_split_weights(dUf, dUp, Uf.size(), usc, s);
            p.pair_scale = 1.0f / (kWinoFused64PairVScale * usc);
            launch_wino_fused64(p, reinterpret_cast<const float*>(dUp), s, r.variant);
            break;
        }
        case ConvPath::Fused32:
        case ConvPath::Fused64:
        case ConvPath::Fused64T: {
            const bool f32k = r.path == ConvPath::Fused32;
            if (f32k ? !wino_fused_eligible(p) : !wino_fused64_eligible(p)) throw HipError("debug_conv: shape not eligible for the fused Winograd kernel");
            const std::vector<float> U = wino_weights(4);
            std::vector<float> Uf(U.size());
            if (f32k) wino_fused_pack_weights(U.data(), Cout, Cin, Uf.data());
            else wino_fused64_pack_weights(U.data(), Cout, Cin, Uf.data());
            float* dUf = mem.upload(Uf);
            if (r.path == ConvPath::Fused64T) {
                if (!wino_fused64t_eligible(p)) throw HipError("debug_conv: shape not eligible for the two-tile-group fused Winograd kernel");
                launch_wino_fused64t(p, dUf, s, r.variant);
            } else if (f32k) {
                launch_wino_fused(p, dUf, s);
            } else {
                launch_wino_fused64(p, dUf, s, r.variant);
            }
            break;
        }
        case ConvPath::WinoF2:
        case ConvPath::WinoF4: {
            const int tile = r.path == ConvPath::WinoF2 ? 2 : 4, ncomp = (tile + 2) * (tile + 2);
            if (!wino_shape_ok(p, tile)) throw HipError("debug_conv: shape not eligible for Winograd");
            const std::vector<float> U = wino_weights(tile);
            const long long T = wino_tiles(tile);
            float* dU = mem.upload(U);
            float* dV = mem.alloc<float>((size_t)ncomp * T * Cin);
            const WinoPlan wp = make_wino(p, dU, dV, alloc_M(ncomp, T), tile);
            launch_wino_input(wp.in, s);
            launch_conv(wp.gemm, s, conv_tune_from_code(r.tune));
            launch_wino_output(wp.out, s);
            break;
        }
        case ConvPath::DirectPair: {
            const bool f16 = r.op == Operand::F16;
            const float sc = f16 ? pow2_scale_into_512(pk.data(), pk.size()) : 1.f;
            unsigned short* dwp = mem.alloc<unsigned short>(2 * pk.size());
            launch_split_pairs(dw, dwp, (size_t)Cout, KH * KW * (C0 + C1), s, f16, sc);
            p.w_pair = dwp; p.pair_scale = 1.0f / sc; p.f16 = f16 ? 1 : 0;
            launch_conv(p, s);
            break;
        }
        case ConvPath::Valu:
            launch_conv_naive(p, s);
            break;
        case ConvPath::Direct: {
            unsigned short* ao = nullptr;
            if (r.op != Operand::F32) {   // bf16- / fp16-MFMA mode
                unsigned short* d16 = mem.alloc<unsigned short>(pk.size());
                if (r.op == Operand::F16) launch_f32_to_f16(dw, d16, pk.size(), s);
                else launch_f32_to_bf16(dw, d16, pk.size(), s);
                p.w_bf = d16;
                p.f16 = r.op == Operand::F16 ? 1 : 0;
            }
            const size_t npix_in = (size_t)B * Hin * Win, nout = (size_t)B * p.Ho * p.Wo * Cout;
            if (r.act_bf16) {  // the caller's fp32 tensors are rounded into bf16 copies; the bf16 result is widened back
                auto to_bf = [&](const float* src, size_t n) {
                    unsigned short* d = mem.alloc<unsigned short>(n + 32);
                    launch_f32_to_bf16(src, d, n, s);
                    return reinterpret_cast<const float*>(d);
                };
                p.in0 = to_bf(in0, npix_in * C0);
                if (in1) p.in1 = to_bf(in1, npix_in * C1);
                if (res) p.res = to_bf(res, nout);
                ao = mem.alloc<unsigned short>(nout + 32);
                p.out = reinterpret_cast<float*>(ao);
                p.in_bf16 = p.out_bf16 = 1;
            }
            launch_conv(p, s, conv_tune_from_code(r.tune));
            if (r.act_bf16) launch_bf16_to_f32(ao, out, nout, s);
            break;
        }
        }
        IRSDE_HIP_CHECK(hipStreamSynchronize(s));
    });
}

int irsde_debug_conv_choice(int B, int Hin, int Win, int C0, int C1, int Cout, int K, int stride, int pad, int in_shift, int operand, int storage, int pair,
                            unsigned features, int splits, int nz, int tune, int cu_count, const int* knobs, char* out, int out_len) {
    return guard([&] {
        if (!out || out_len < 1 || K < 1 || stride < 1 || cu_count < 1 || operand < 0 || operand > 2 || storage < 0 || storage > 2 || (pair && operand == 0))
            throw HipError("debug_conv_choice: bad argument");
        const ConvParams p = choice_hook_params(B, Hin, Win, C0, C1, Cout, K, stride, pad, in_shift, operand, storage, pair, features, splits, nz);
        ConvKnobs k;
        static_assert(sizeof(ConvKnobs) == 11 * sizeof(int), "the hook's knob array is ConvKnobs, field by field");
        if (knobs) memcpy(&k, knobs, sizeof k);
        conv_validate(p);
        const ConvChoice c = conv_choose(p, conv_tune_from_code(tune), k, cu_count);
        const bool tabled = c.family != ConvChoice::NARROW3 && c.family != ConvChoice::HALO;
        if (tabled && c.row < 0) throw HipError("launch_conv: no kernel instance " + c.name());
        write_choice_line(c, out, out_len);
    });
}

int irsde_debug_conv_halo_choice(int B, int Hin, int Win, int C0, int C1, int Cout, int K, int stride, int pad, int in_shift, int operand, int storage, int pair,
                                 unsigned features, int splits, int nz, int tune, int halo2, int nslow, char* out, int out_len) {
    return guard([&] {
        if (!out || out_len < 1 || K < 1 || stride < 1 || operand < 0 || operand > 2 || storage < 0 || storage > 2 || (pair && operand == 0))
            throw HipError("debug_conv_halo_choice: bad argument");
        const ConvParams p = choice_hook_params(B, Hin, Win, C0, C1, Cout, K, stride, pad, in_shift, operand, storage, pair, features, splits, nz);
        conv_validate(p);
        const ConvTune t = conv_tune_from_code(tune);
        // (no branch that conv_choose tries before the halo family takes a layer the family would: they want w_pair, f32 operands or nz > 1; the CU
        //  count and the knobs do not reach this choice)
        const ConvChoice c = conv_choose(p, t, ConvKnobs{}, 256);
        if (c.family != ConvChoice::HALO) throw HipError("debug_conv_halo_choice: conv_choose does not send this layer to the halo family, but to " + c.name());
        write_halo_line(conv_halo_choose(p, t, halo2, nslow), out, out_len);
    });
}

int irsde_debug_conv_features(const float* in0, int C0, const float* in1, int C1, int B, int Hin, int Win, int in_shift, const float* w_oihw, int Cout, int K,
                              int stride, int pad, int operand, int storage, int pair, const float* bias, const float* ch_scale, const float* ln_g,
                              const float* film, int film_bstride, const float* res, const float* in_scale, const float* gate_film, int gate_film_bstride,
                              int silu, int gate, int shuffle, int nz, int splits, int tune, const int* knobs, float* out, char* choice, int choice_len,
                              void* stream) {
    return guard([&] {
        if (!in0 || !w_oihw || !out || !choice || choice_len < 1) throw HipError("null argument");
        if (B < 1 || Hin < 1 || Win < 1 || C0 < 1 || C1 < 0 || (C1 > 0) != (in1 != nullptr) || Cout < 1 || K < 1 || stride < 1 || pad < 0 || in_shift < 0 || in_shift > 1 ||
            operand < 0 || operand > 2 || storage < 0 || storage > 2 || (pair && operand == 0) || nz < 1 || splits < 1 || film_bstride < 0 || gate_film_bstride < 0)
            throw HipError("debug_conv_features: bad argument");
        if ((gate && shuffle) || (gate && (Cout % 4 || res)) || (shuffle && Cout % 4) || (gate_film && !gate) || ((gate || shuffle) && film))
            throw HipError("debug_conv_features: gate needs Cout % 4 == 0 and takes no residual, shuffle needs Cout % 4 == 0, gate_film goes with gate, film with neither");
        if (nz > 1 && (B != 1 || Hin != 1 || K != 1 || stride != 1 || pad || in_shift || C1 || storage))
            throw HipError("debug_conv_features: nz > 1 is a stack of 1x1 GEMMs: B = 1, Hin = 1, K = 1, one fp32 source");
        const int Ho = ((Hin << in_shift) + 2 * pad - K) / stride + 1, Wo = ((Win << in_shift) + 2 * pad - K) / stride + 1;
        if (Ho < 1 || Wo < 1) throw HipError("debug_conv_features: empty output");
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        conv_global_init();
        const int Cin = C0 + C1;
        // the engine's own packing, component by component: conv4's gate pairs, ups.i.0's pixel-shuffle order, else the identity
        const std::vector<int> perm = gate ? naf_gate_perm(Cout / 2) : shuffle ? naf_shuffle_perm(Cout) : std::vector<int>();
        const size_t wz = (size_t)Cout * K * K * Cin;
        std::vector<float> pk(wz * nz), pb, one, oneb;
        for (int z = 0; z < nz; ++z) {
            pack_conv_rows(w_oihw + z * wz, z == 0 ? bias : nullptr, Cout, Cin, K, K, perm, one, z == 0 ? pb : oneb);
            std::copy(one.begin(), one.end(), pk.begin() + z * wz);
        }
        Scratch mem(s);
        float* dw = mem.upload(pk);
        ConvParams p;
        p.in0 = in0; p.C0 = C0; p.pix0 = C0; p.in1 = in1; p.C1 = C1; p.pix1 = C1;
        p.Hin = Hin; p.Win = Win; p.in_shift = in_shift;
        p.w = dw; p.Cout = Cout; p.KH = K; p.KW = K; p.stride = stride; p.pad_y = pad; p.pad_x = pad;
        p.B = B; p.Ho = Ho; p.Wo = Wo;
        const int ostride = gate ? Cout / 2 : shuffle ? Cout / 4 : Cout;
        const size_t npix_in = (size_t)B * Hin * Win * nz, M = (size_t)B * Ho * Wo, nout = M * nz * (gate ? Cout / 2 : Cout);
        p.out = out; p.out_stride = ostride; p.res = res; p.res_stride = ostride;
        if (bias) p.bias = mem.upload(pb);
        if (ch_scale) {   // (a row vector of the packed rows, like the bias)
            std::vector<float> cs(Cout);
            for (int o = 0; o < Cout; ++o) cs[o] = ch_scale[perm.empty() ? o : perm[o]];
            p.ch_scale = mem.upload(cs);
        }
        if (ln_g) p.ln_g = mem.upload(ln_g, Cout);
        p.film = film; p.film_bstride = film_bstride; p.silu = silu; p.in_scale = in_scale;
        p.gate = gate ? 1 : 0; p.gate_film = gate_film; p.gate_film_bstride = gate_film ? gate_film_bstride : 0; p.shuffle = shuffle ? 1 : 0;
        p.nz = nz;
        if (nz > 1) { p.z_in = (long long)Win * C0; p.z_w = (long long)Cout * C0; p.z_out = (long long)Win * Cout; }
        float* dz = mem.alloc<float>(256);
        IRSDE_HIP_CHECK(hipMemset(dz, 0, 1024));
        p.zeros = dz;
        if (splits > 1) {
            p.splits = splits;
            p.partial = mem.alloc<float>((size_t)splits * M * Cout);
        }
        const bool f16 = operand == 2;
        unsigned short *w16 = nullptr, *a0 = nullptr, *a1 = nullptr, *ar = nullptr, *ao = nullptr;
        float wsc = 1.f;
        if (pair) {
            wsc = f16 ? pow2_scale_into_512(pk.data(), pk.size()) : 1.f;
            w16 = mem.alloc<unsigned short>(2 * pk.size());
            p.w_pair = w16; p.pair_scale = 1.0f / wsc;
        } else if (operand) {
            w16 = mem.alloc<unsigned short>(pk.size());
            p.w_bf = w16;
        }
        p.f16 = f16 ? 1 : 0;
        if (storage) {   // the caller's fp32 tensors are rounded into 16-bit copies of the same extents; the 16-bit result is widened back
            a0 = mem.alloc<unsigned short>(npix_in * C0);
            p.in0 = reinterpret_cast<const float*>(a0);
            if (in1) { a1 = mem.alloc<unsigned short>(npix_in * C1); p.in1 = reinterpret_cast<const float*>(a1); }
            if (res) { ar = mem.alloc<unsigned short>(nout); p.res = reinterpret_cast<const float*>(ar); }
            ao = mem.alloc<unsigned short>(nout);
            p.out = reinterpret_cast<float*>(ao);
            p.in_bf16 = p.out_bf16 = storage == 1;
            p.in_f16 = p.out_f16 = storage == 2;
        }
        ConvKnobs k;
        static_assert(sizeof(ConvKnobs) == 11 * sizeof(int), "the hook's knob array is ConvKnobs, field by field");
        if (knobs) memcpy(&k, knobs, sizeof k);
        conv_validate(p);   // every refusal before the first launch, the hook's own conversions included
        auto narrow = [&](const float* src, unsigned short* dst, size_t n) {
            if (storage == 2) launch_f32_to_f16(src, dst, n, s);
            else launch_f32_to_bf16(src, dst, n, s);
        };
        if (pair) launch_split_pairs(dw, w16, (size_t)Cout * nz, K * K * Cin, s, f16, wsc);
        else if (operand == 2) launch_f32_to_f16(dw, w16, pk.size(), s);
        else if (operand == 1) launch_f32_to_bf16(dw, w16, pk.size(), s);
        if (storage) {
            narrow(in0, a0, npix_in * C0);
            if (in1) narrow(in1, a1, npix_in * C1);
            if (res) narrow(res, ar, nout);
            IRSDE_HIP_CHECK(hipMemsetAsync(ao, 0xFF, nout * 2, s));   // NaN in both 16-bit formats: an element the kernel leaves out stays visible after the widening
        }
        ConvChoice c;
        launch_conv(p, s, conv_tune_from_code(tune), knobs ? &k : nullptr, &c);
        if (storage == 2) launch_f16_to_f32(ao, out, nout, s);
        else if (storage == 1) launch_bf16_to_f32(ao, out, nout, s);
        IRSDE_HIP_CHECK(hipStreamSynchronize(s));
        write_choice_line(c, choice, choice_len);
        if (c.family == ConvChoice::HALO) {   // + the halo path's own choice for this launch
            const size_t n = strlen(choice);
            if (n + 2 < (size_t)choice_len) {
                choice[n] = ' ';
                write_halo_line(c.halo, choice + n + 1, choice_len - (int)n - 1);
            }
        }
    });
}

int irsde_debug_split_gemm(const float* A, const float* Bm, float* C, int M, int N, int K, int ncomp, int nplanes, void* stream) {
    return guard([&] {
        // 42 / 44: the engine's pair-interleaved two-plane kernel on bf16 / fp16 pieces
        // 43: the exact-fp32 engine's three-piece kernel (row-pair-interleaved triples, six products) on its production launch (the persistent item walk);
        // 45: the same kernel on the one-item-per-block launch, the walk's bit-identity twin; 47: the walk with vmcnt(0) in front of every barrier, the ring's twin
        const int twin3 = nplanes == 43 ? 0 : nplanes == 45 ? 1 : nplanes == 47 ? 2 : -1;   // split3_launch_twin
        if (twin3 < 0 && nplanes != 42 && nplanes != 44) throw HipError("debug_split_gemm: nplanes must be 42, 43, 44, 45 or 47");
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        conv_global_init();
        Scratch mem(s);
        if (twin3 >= 0) {
            if (!gemm_split_triples_fits(M, N, K, N)) throw HipError("debug_split_gemm: shape not eligible for the three-piece GEMM");
            launch_gemm_split_triples(split_triples(mem, A, Bm, C, M, N, K, ncomp, s), ncomp, s, split3_launch_twin(twin3));
        } else {   // (fp16: any powers of two, the hook exercises the scaling)
            const bool f16 = nplanes == 44;
            launch_gemm_split_pairs(split_pairs(mem, A, Bm, C, M, N, K, ncomp, s, f16, f16 ? 1.0f / 16.0f : 1.f, f16 ? 64.0f : 1.f), ncomp, s, 0, f16);
        }
        IRSDE_HIP_CHECK(hipStreamSynchronize(s));
    });
}

int irsde_debug_force_chain_groups(int g) {
    set_force_chain_groups(g == 1 || g == 2 || g == 4 ? g : 0);
    return IRSDE_OK;
}

int irsde_debug_force_split3(int mode) {
    set_force_split3(mode >= 0 && mode <= 2 ? mode : -1);
    return IRSDE_OK;
}

int irsde_debug_force_split3_attn(int mode) {
    set_force_split3_attn(mode >= 0 && mode <= 2 ? mode : -1);
    return IRSDE_OK;
}
int irsde_debug_force_split3_1x1(int mode) {
    set_force_split3_1x1(mode >= 0 && mode <= 2 ? mode : -1);
    return IRSDE_OK;
}

int irsde_debug_split3_1x1(const float* in0, int C0, int pix0, const float* in1, int C1, int pix1, const float* w, const float* bias, float* out, int M, int N,
                           int out_stride, int mode, void* stream) {
    return guard([&] {
        if (!in0 || !w || !out || (C1 && !in1) || mode < 0 || mode > 2) throw HipError("debug_split3_1x1: bad argument");
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        conv_global_init();
        Split3aArgs a;
        a.in0 = in0; a.C0 = C0; a.pix0 = pix0; a.in1 = C1 ? in1 : nullptr; a.C1 = C1; a.pix1 = C1 ? pix1 : 0;
        a.bias = bias; a.out = out; a.M = M; a.N = N; a.out_stride = out_stride;
        const char* why = nullptr;
        if (!gemm_split3a_fits(a, &why)) throw HipError(std::string("debug_split3_1x1: ") + why);
        Scratch mem(s);
        unsigned short* wt = mem.alloc<unsigned short>(split3_comp_elems((size_t)N, (size_t)(C0 + C1)));
        launch_split_triples(w, wt, 1, (size_t)N, C0 + C1, s);
        a.w3 = wt;
        launch_gemm_split3a(a, s, split3_launch_twin(mode));
        IRSDE_HIP_CHECK(hipStreamSynchronize(s));
    });
}

int irsde_debug_split3_1x1_choice(int B, int Hin, int Win, int C0, int C1, int Cout, int K, int stride, int pad, int in_shift, int operand, int storage, int pair,
                                  unsigned features, int splits, int nz, int engine_flags, int master, int knob, int cu_count, char* out, int out_len) {
    return guard([&] {
        if (!out || out_len < 1 || K < 1 || stride < 1 || cu_count < 1 || operand < 0 || operand > 2 || storage < 0 || storage > 2 || (pair && operand == 0))
            throw HipError("debug_split3_1x1_choice: bad argument");
        const ConvParams p = choice_hook_params(B, Hin, Win, C0, C1, Cout, K, stride, pad, in_shift, operand, storage, pair, features, splits, nz);
        const Split3x1Choice c = split3_1x1_choose(p, !(engine_flags & kSplit3NotExactF32), master, knob, cu_count);
        snprintf(out, (size_t)out_len, "adopt=%d grid=%d lds=%d why_not=%s", c.adopt ? 1 : 0, c.grid, c.lds, c.why_not);
    });
}

int irsde_debug_force_split3_blocks(int n) {
    if (n >= 0 && n < 8) return guard([&] { throw HipError("debug_force_split3_blocks: n must be at least 8 (one block per XCD), or negative for the default"); });
    set_force_split3_blocks(n);
    return IRSDE_OK;
}

int irsde_debug_force_wino_poly(int mode) {
    set_force_wino_poly(mode >= 0 && mode <= 2 ? mode : -1);
    return IRSDE_OK;
}

int irsde_debug_force_subbatches(int n) {
    set_force_subbatches(n < 0 ? 0 : n);
    return IRSDE_OK;
}

int irsde_bench_naf_chain(int variant, int nblocks, int B, int iters, double* ms_out) {
    return guard([&] {
        if (!ms_out || nblocks < 1 || nblocks > 64 || B < 1 || iters < 1) throw HipError("bench_naf_chain: bad argument");
        // 0 / 1 production; 11 (PROBES build) its cycle stamps; r06: 22 / 24 = the kernel with 2 / 4 work-groups per image, 25 (PROBES build) 24 + its cycle
        // stamps, 26 (PROBES build) 24 with one group per image missing — must report the spin timeout
        const int G = variant == 22 ? 2 : (variant == 24 || variant == 25 || variant == 26) ? 4 : 1;
#ifdef IRSDE_PROBES
        if (variant != 0 && variant != 1 && variant != 11 && G == 1) throw HipError("bench_naf_chain: bad variant");
#else
        if (variant != 0 && variant != 1 && G == 1) throw HipError("bench_naf_chain: variant 11 is a measurement twin (make PROBES=1)");   // (before anything is allocated)
#endif
        conv_global_init();
        OwnedStream stream(hipStreamDefault);
        hipStream_t s = stream.s;
        Scratch mem(s);
        const size_t nx = (size_t)B * 64 * 512, nw = naf_chain_weight_halves(nblocks), nv = naf_chain_vec_floats(nblocks);
        float *dx = mem.alloc<float>(nx), *dout = mem.alloc<float>(nx), *dvec = mem.alloc<float>(nv), *dfilm = mem.alloc<float>((size_t)nblocks * 2048);
        unsigned short* dw = mem.alloc<unsigned short>(nw);
        const size_t chunk = (size_t)64 << 20;   // f32 staging of the random weights, converted to fp16 piecewise
        float* dwf = mem.alloc<float>(chunk);
        launch_fill_random(dx, nx, 1, 1.0f, s);
        launch_fill_random(dvec, nv, 2, 0.1f, s);
        launch_fill_random(dfilm, (size_t)nblocks * 2048, 3, 0.1f, s);
        for (size_t o = 0; o < nw; o += chunk) {
            const size_t n = std::min(chunk, nw - o);
            launch_fill_random(dwf, n, 4 + (unsigned)(o / chunk), 0.04f, s);
            launch_f32_to_f16(dwf, dw + o, n, s);
        }
        unsigned short* dwg = nullptr;
        void* dscratch = nullptr;
        if (G > 1) {
            IRSDE_HIP_CHECK(hipStreamSynchronize(s));
            dwg = mem.alloc<unsigned short>(nw);
            naf_chain_build_split_weights(dw, dwg, nblocks, G, s);
            dscratch = mem.alloc<char>(naf_chain_split_scratch_bytes(B));
            IRSDE_HIP_CHECK(hipMemset(dscratch, 0, naf_chain_split_scratch_bytes(B)));
        }
        auto run = [&]() {
            if (G > 1) launch_naf_chain_split(dx, dout, dwg, dvec, nblocks, B, dfilm, 0, 0, nullptr, 0, 0, G, dscratch, s);
            else launch_naf_chain(dx, dout, dw, dvec, nblocks, B, dfilm, 0, 0, nullptr, 0, 0, s, variant == 11 ? 1 : variant);
        };
        if (variant == 26) {
#ifdef IRSDE_PROBES
            naf_chain_set_sabotage(1);
#else
            throw HipError("bench_naf_chain: variant 26 is a PROBES-build test");
#endif
        }
        struct SabotageOff { ~SabotageOff() { naf_chain_set_sabotage(0); } } sabotage_off;
        run();   // warm
        if (variant == 25) {
#ifdef IRSDE_PROBES
            const int ng = naf_chain_split_groups(B, 4);
            unsigned long long* dd = mem.alloc<unsigned long long>((size_t)ng * 8 * 16);
            IRSDE_HIP_CHECK(hipMemsetAsync(dd, 0, (size_t)ng * 8 * 16 * 8, s));
            naf_chain_set_debug(dd);
            run();
            IRSDE_HIP_CHECK(hipStreamSynchronize(s));
            naf_chain_set_debug(nullptr);
            std::vector<unsigned long long> hd((size_t)ng * 8 * 16);
            IRSDE_HIP_CHECK(hipMemcpy(hd.data(), dd, hd.size() * 8, hipMemcpyDeviceToHost));
            double acc[16] = {0};
            double nwv = 0;
            for (size_t w = 0; w < (size_t)ng * 8; ++w) {
                if (!hd[w * 16 + 15]) continue;   // (a group of an image slot past the batch)
                for (int k = 0; k < 16; ++k) acc[k] += (double)hd[w * 16 + k];
                nwv += 1;
            }
            static const char* names[12] = {"norm1 (incl. residual-stream fetch)", "conv1 GEMM passes", "depthwise 3x3 + gate + pool", "gated fetch behind barrier (pool)", "sca.1 GEMM", "conv3 GEMM + residual", "norm2 (incl. residual-stream fetch)", "conv4 GEMM + gate", "conv5 GEMM + residual", "scale-vector / gated fetch (sca, conv4)", "group barriers (6 per block)", "publishing (gated slice, residual slice)"};
            printf("naf_chain stamps, 4 groups per image: %d blocks, B=%d; shader cycles per wave and block (mean over %.0f waves)\n", nblocks, B, nwv);
            for (int k = 0; k < 12; ++k) printf("  %-42s %9.0f\n", names[k], acc[k] / nwv / nblocks);
            printf("  %-42s %9.0f\n", "whole kernel / blocks", acc[15] / nwv / nblocks);
            fflush(stdout);
#else
            throw HipError("bench_naf_chain: variant 25 is a measurement twin (make PROBES=1)");
#endif
        }
        if (variant == 11) {   // the stamp twin once: per-phase cycle budget per block, averaged over all waves
            unsigned long long* dd = mem.alloc<unsigned long long>((size_t)B * 8 * 16);
            IRSDE_HIP_CHECK(hipMemsetAsync(dd, 0, (size_t)B * 8 * 16 * 8, s));
            naf_chain_set_debug(dd);
            launch_naf_chain(dx, dout, dw, dvec, nblocks, B, dfilm, 0, 0, nullptr, 0, 0, s, 11);
            IRSDE_HIP_CHECK(hipStreamSynchronize(s));
            naf_chain_set_debug(nullptr);
            std::vector<unsigned long long> hd((size_t)B * 8 * 16);
            IRSDE_HIP_CHECK(hipMemcpy(hd.data(), dd, hd.size() * 8, hipMemcpyDeviceToHost));
            double acc[16] = {0};
            for (size_t i = 0; i < hd.size(); ++i) acc[i % 16] += (double)hd[i];
            const double nwv = (double)B * 8, nb = nblocks;
            static const char* names[10] = {"norm1", "conv1 GEMM passes", "depthwise 3x3 + gate + pool", "barrier (pool)", "sca.1 GEMM", "conv3 GEMM + residual", "norm2", "conv4 GEMM + gate", "conv5 GEMM + residual", "barriers (sca, conv4)"};
            printf("naf_chain stamps: %d blocks, B=%d; shader cycles per wave and block (mean over %d waves); MFMA floor per wave: conv1 / conv4 512 x 16, conv3 / conv5 256 x 16, sca 64 x 16\n", nblocks, B, B * 8);
            for (int k = 0; k < 10; ++k) printf("  %-30s %9.0f\n", names[k], acc[k] / nwv / nb);
            printf("  %-30s %9.0f\n", "whole kernel / blocks", acc[15] / nwv / nb);
            fflush(stdout);
        }
        *ms_out = time_launches(s, iters, run);
        if (G > 1) {
            unsigned flag = 0;
            IRSDE_HIP_CHECK(hipMemcpy(&flag, naf_chain_split_error_flag(dscratch, B), 4, hipMemcpyDeviceToHost));
            if (flag) throw HipError("bench_naf_chain: the split kernel's groups were not co-resident (spin timeout)");
        }
    });
}

int irsde_bench_conv(int variant, int B, int H, int W, int Cin, int Cout, int K, int stride, int up, int epi, int iters,
                     double* ms_out) {
    return guard([&] {
        if (!ms_out || iters < 1) throw HipError("bad argument");
        const BenchSel sel = bench_conv_lookup(variant);
        const BenchRow& r = sel.row;
        const BenchKind kind = r.kind;
        const int arg = sel.arg;
        conv_global_init();
        OwnedStream stream(hipStreamNonBlocking);
        hipStream_t s = stream.s;
        Scratch mem(s);
        ConvParams p;
        p.B = B; p.Hin = H; p.Win = W; p.in_shift = up; p.C0 = Cin; p.pix0 = Cin;
        p.Cout = Cout; p.KH = K; p.KW = K; p.stride = stride; p.pad_y = p.pad_x = (K == 4 ? 1 : K / 2);
        p.Ho = ((H << up) + 2 * p.pad_y - K) / stride + 1;
        p.Wo = ((W << up) + 2 * p.pad_x - K) / stride + 1;
        const size_t nin = (size_t)B * H * W * Cin, nw = (size_t)Cout * K * K * Cin, nout = (size_t)B * p.Ho * p.Wo * Cout;
        float *din = mem.alloc<float>(nin), *dw = mem.alloc<float>(nw), *dout = mem.alloc<float>(nout), *dres = mem.alloc<float>(nout);
        float* dfilm = mem.alloc<float>((size_t)2 * Cout + 256);   // + the zero page
        float* dz = dfilm + 2 * Cout;
        IRSDE_HIP_CHECK(hipMemset(dz, 0, 1024));
        p.zeros = dz;
        launch_fill_random(din, nin, 1, 1.0f, s);
        launch_fill_random(dw, nw, 2, 1.0f / sqrtf((float)(K * K * Cin)), s);
        launch_fill_random(dres, nout, 3, 1.0f, s);
        launch_fill_random(dfilm, (size_t)2 * Cout, 4, 0.3f, s);
        p.in0 = din; p.w = dw; p.out = dout; p.out_stride = Cout;
        if (kind == BenchKind::Conv && r.op == Operand::BF16 && !r.pair) {  // bf16-MFMA mode
            unsigned short* dbf = mem.alloc<unsigned short>(nw);
            launch_f32_to_bf16(dw, dbf, nw, s);
            p.w_bf = dbf;
        }
        if (epi == 1) { p.film = dfilm; p.silu = 1; }
        if (epi == 2) { p.silu = 1; p.res = dres; p.res_stride = Cout; }
        if (r.act_bf16) {  // bf16 activation storage (the output / residual buffers are simply twice the size needed)
            unsigned short* dabf = mem.alloc<unsigned short>(nin);
            launch_f32_to_bf16(din, dabf, nin, s);
            launch_f32_to_bf16(dout, reinterpret_cast<unsigned short*>(dres), nout / 2, s);
            p.in0 = reinterpret_cast<const float*>(dabf);
            p.in_bf16 = 1; p.out_bf16 = 1;
        }
        if (r.pair) {   // direct convolution on the PAIR kernels
            const bool f16 = r.op == Operand::F16;
            unsigned short* dwp = mem.alloc<unsigned short>(2 * nw);
            launch_split_pairs(dw, dwp, (size_t)Cout, K * K * Cin, s, f16, 64.0f);
            p.w_pair = dwp; p.pair_scale = 1.0f / 64.0f; p.f16 = f16 ? 1 : 0;
        }
        if (kind == BenchKind::Split3aGemm) {   // the layer on gemm_split3a_kernel alone (weights split ahead of the timed launches)
            const Split3x1Choice c = split3_1x1_choose(p, true, 2, 2, device_cu_count());
            if (!c.adopt || up || epi) throw HipError(std::string("bench_conv: variants 510 - 524 run a plain 1x1 layer: ") + (c.adopt ? "no epilogue" : c.why_not));
            unsigned short* dwt = mem.alloc<unsigned short>(split3_comp_elems((size_t)Cout, (size_t)Cin));
            launch_split_triples(dw, dwt, 1, (size_t)Cout, Cin, s);
            const Split3aArgs a = split3_1x1_args(p, dwt);
            const Split3Launch twin = split3_launch_twin(arg / 5, arg % 5);
            for (int i = 0; i < 2; ++i) launch_gemm_split3a(a, s, twin);
            *ms_out = time_launches(s, iters, [&] { launch_gemm_split3a(a, s, twin); });
            return;
        }
        if (kind == BenchKind::TripleGemm || kind == BenchKind::PairGemm) {   // the 36 component GEMMs of the layer alone, on random operands
            if (K != 3 || stride != 1 || !wino_shape_ok(p, 4)) throw HipError("bench_conv: Winograd variants need an eligible 3x3 stride-1 layer");
            const long long T = (long long)B * (p.Ho / 4) * (p.Wo / 4);
            const bool triples = kind == BenchKind::TripleGemm;
            if (triples && !gemm_split_triples_fits(T, Cout, Cin, Cout)) throw HipError("bench_conv: shape not eligible for the three-piece GEMM");
            float *vf = mem.alloc<float>((size_t)36 * T * Cin), *uf = mem.alloc<float>((size_t)36 * Cout * Cin), *mo = mem.alloc<float>((size_t)36 * T * Cout);
            launch_fill_random(vf, (size_t)36 * T * Cin, 7, 1.0f, s);
            launch_fill_random(uf, (size_t)36 * Cout * Cin, 8, 0.05f, s);
            const SplitGemmArgs g = triples ? split_triples(mem, vf, uf, mo, (int)T, Cout, Cin, 36, s) : split_pairs(mem, vf, uf, mo, (int)T, Cout, Cin, 36, s);
            const Split3Launch twin = split3_launch_twin(arg / 5, arg % 5);
            auto gemms = [&] {
                if (triples) launch_gemm_split_triples(g, 36, s, twin);
                else launch_gemm_split_pairs(g, 36, s, arg);
            };
            for (int i = 0; i < 2; ++i) gemms();
            *ms_out = time_launches(s, iters, gemms);
            return;
        }
        float* dU = nullptr;
        WinoPlan wp{};
        if (kind == BenchKind::Fused32Stamps) {  // fused Winograd kernel once, with per-wave phase stamps: prints the averaged timeline
            dU = mem.alloc<float>((size_t)36 * nw / 9);
            launch_fill_random(dU, (size_t)36 * nw / 9, 5, 1.0f / sqrtf((float)(9 * Cin)), s);
            const int nb = wino_fused_num_blocks(p);
            unsigned long long* dd = mem.alloc<unsigned long long>((size_t)nb * 128);
            launch_wino_fused(p, dU, s);  // warm
            IRSDE_HIP_CHECK(hipMemsetAsync(dd, 0, (size_t)nb * 128 * 8, s));
            launch_wino_fused(p, dU, s, dd);
            IRSDE_HIP_CHECK(hipStreamSynchronize(s));
            std::vector<unsigned long long> hd((size_t)nb * 128);
            IRSDE_HIP_CHECK(hipMemcpy(hd.data(), dd, hd.size() * 8, hipMemcpyDeviceToHost));
            double ph[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
            unsigned long long rt_min = ~0ull, rt_max = 0;
            for (int bi = 0; bi < nb; ++bi)
                for (int w = 0; w < 8; ++w) {
                    const unsigned long long* t = &hd[((size_t)bi * 8 + w) * 16];
                    for (int k = 0; k < 4; ++k) ph[w >= 4][k] += (double)(t[k + 1] - t[k]) / ((double)nb * 4);
                    rt_min = std::min(rt_min, t[7]);
                    rt_max = std::max(rt_max, t[7]);
                }
            // block start times (100 MHz realtime counter) -> how long the launch kept dispatching new blocks
            printf("wino_fused timeline B=%d %dx%d Cin=%d Cout=%d: %d blocks, block starts span %.1f us\n", B, p.Ho, p.Wo, Cin, Cout, nb,
                   (double)(rt_max - rt_min) / 100.0);
            printf("  MFMA waves     (shader cycles): start->V[0] ready %.0f | K loop %.0f | acc->LDS+barrier %.0f | epilogue %.0f\n", ph[0][0],
                   ph[0][1], ph[0][2], ph[0][3]);
            printf("  producer waves (shader cycles): start->chunk 0 done %.0f | K loop rest %.0f | wait MFMA+acc %.0f | epilogue %.0f\n",
                   ph[1][0], ph[1][1], ph[1][2], ph[1][3]);
            fflush(stdout);
            *ms_out = 0.0;
            return;
        }
        if (kind != BenchKind::Conv) {   // the Winograd kinds: random U (timing only)
            const bool three_launch = kind == BenchKind::Wino3 || kind == BenchKind::Wino3Gemm;
            if (K != 3 || stride != 1) throw HipError("bench_conv: Winograd variants need a 3x3 stride-1 layer");
            dU = mem.alloc<float>((size_t)36 * nw / 9);
            launch_fill_random(dU, (size_t)36 * nw / 9, 5, 1.0f / sqrtf((float)(9 * Cin)), s);
            if (!three_launch && !wino_fused_eligible(p)) throw HipError("bench_conv: shape not eligible for the fused Winograd kernel");
            // (the GEMMs-alone variant is held to the 64-cout kernel's shapes too: it is timed next to those kernels)
            if (kind != BenchKind::Fused32 && kind != BenchKind::Wino3 && !wino_fused64_eligible(p))
                throw HipError("bench_conv: shape not eligible for the 64-cout fused Winograd kernel");
            if (kind == BenchKind::Fused64 && r.op == Operand::F16) {  // the fp16-pair kernel: the random weights as hi / lo halves
                float* dUp = mem.alloc<float>((size_t)36 * nw / 9);
                launch_wino_fused64_split_weights(dU, reinterpret_cast<unsigned short*>(dUp), (size_t)36 * nw / 9, 256.0f, s);
                dU = dUp;
                p.pair_scale = 1.0f / (kWinoFused64PairVScale * 256.0f);
            }
            if (three_launch) {
                if (!wino_shape_ok(p, 4)) throw HipError("bench_conv: shape not eligible for Winograd F(4x4,3x3)");
                const long long T = (long long)B * (p.Ho / 4) * (p.Wo / 4);
                float* dV = mem.alloc<float>((size_t)36 * T * Cin);
                float* dM = mem.alloc<float>((size_t)36 * T * Cout);
                wp = make_wino(p, dU, dV, dM, 4);
                if (kind == BenchKind::Wino3Gemm) launch_wino_input(wp.in, s);
            }
        }
        if (kind == BenchKind::Fused64TStamps) {   // r06: the two-tile-group kernel once with per-wave cycle stamps
            if (!wino_fused64t_eligible(p)) throw HipError("bench_conv: shape not eligible for the two-tile-group fused Winograd kernel");
            const int nbp = 256;
            unsigned long long* dd = mem.alloc<unsigned long long>((size_t)nbp * 64);
            launch_wino_fused64t(p, dU, s, 0);  // warm
            IRSDE_HIP_CHECK(hipMemsetAsync(dd, 0, (size_t)nbp * 64 * 8, s));
            wino_fused64t_set_debug(dd);
            launch_wino_fused64t(p, dU, s, arg);
            IRSDE_HIP_CHECK(hipStreamSynchronize(s));
            wino_fused64t_set_debug(nullptr);
            std::vector<unsigned long long> hd((size_t)nbp * 64);
            IRSDE_HIP_CHECK(hipMemcpy(hd.data(), dd, hd.size() * 8, hipMemcpyDeviceToHost));
            double a5[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            int nwv = 0;
            for (int bi = 0; bi < nbp; ++bi)
                for (int w = 0; w < 8; ++w) {
                    const unsigned long long* t = &hd[((size_t)bi * 8 + w) * 8];
                    if (!t[3]) continue;
                    for (int k = 0; k < 8; ++k) a5[k] += (double)t[k];
                    nwv++;
                }
            const int nst = Cin / 16;
            const double items = a5[4] / std::max(nwv, 1), chunks = items * nst;
            printf("wino4_fused64t stamps B=%d %dx%d Cin=%d Cout=%d: %.1f items x %d chunks of 16 channels per block; shader cycles per wave (mean over %d waves)\n", B, p.Ho, p.Wo, Cin,
                   Cout, items, nst, nwv);
            printf("  kernel %.0f = K loops incl. transform slices %.0f (%.0f per chunk; MFMA floor per SIMD 9216) + chunk barrier waits %.0f (%.0f per chunk) + epilogue, exchange, first-chunk transform %.0f (%.0f per item)\n",
                   a5[3] / nwv, a5[0] / nwv, a5[0] / nwv / chunks, a5[1] / nwv, a5[1] / nwv / chunks, (a5[2] + a5[5] + a5[6] + a5[7]) / nwv, (a5[2] + a5[5] + a5[6] + a5[7]) / nwv / items);
            printf("  per item: first stage + exchange writes + ring %.0f | exchange barriers + reads %.0f | second stage, stores, gathers %.0f | zero, first-chunk transform, barrier %.0f\n",
                   a5[5] / nwv / items, a5[6] / nwv / items, a5[7] / nwv / items, a5[2] / nwv / items);
            fflush(stdout);
            *ms_out = 0.0;
            return;
        }
        if (kind == BenchKind::Fused64Stamps) {  // the persistent fused Winograd kernel once with per-wave cycle stamps: prints the averaged budget
            const int nbp = 256;
            unsigned long long* dd = mem.alloc<unsigned long long>((size_t)nbp * 64);
            launch_wino_fused64(p, dU, s, 20);  // warm
            IRSDE_HIP_CHECK(hipMemsetAsync(dd, 0, (size_t)nbp * 64 * 8, s));
            wino_fused64_set_debug(dd);
            launch_wino_fused64(p, dU, s, arg);
            IRSDE_HIP_CHECK(hipStreamSynchronize(s));
            wino_fused64_set_debug(nullptr);
            std::vector<unsigned long long> hd((size_t)nbp * 64);
            IRSDE_HIP_CHECK(hipMemcpy(hd.data(), dd, hd.size() * 8, hipMemcpyDeviceToHost));
            double acc[2][5] = {{0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}};
            int nw[2] = {0, 0};
            for (int bi = 0; bi < nbp; ++bi)
                for (int w = 0; w < 8; ++w) {
                    const unsigned long long* t = &hd[((size_t)bi * 8 + w) * 8];
                    if (!t[3]) continue;
                    for (int k = 0; k < 5; ++k) acc[w >= 4][k] += (double)t[k];
                    nw[w >= 4]++;
                }
            const int nchk = Cin / 32;
            const double items = acc[0][4] / std::max(nw[0], 1), chunks = acc[1][4] / std::max(nw[1], 1);
            printf("wino4_fused64p stamps B=%d %dx%d Cin=%d Cout=%d: %.1f items x %d chunks per block; shader cycles per wave (mean over %d + %d waves)\n", B, p.Ho, p.Wo,
                   Cin, Cout, items, nchk, nw[0], nw[1]);
            printf("  MFMA waves    : kernel %.0f = K-loop compute %.0f (%.0f per chunk; MFMA floor 9216) + barrier wait %.0f (%.0f per chunk) + epilogue %.0f (%.0f per item)\n",
                   acc[0][3] / nw[0], acc[0][0] / nw[0], acc[0][0] / nw[0] / (items * nchk), acc[0][1] / nw[0], acc[0][1] / nw[0] / (items * nchk), acc[0][2] / nw[0],
                   acc[0][2] / nw[0] / items);
            printf("  producer waves: kernel %.0f = load issue %.0f (%.0f per chunk) + data wait, transform, LDS writes %.0f (%.0f per chunk) + barrier wait %.0f (%.0f per chunk)\n",
                   acc[1][3] / nw[1], acc[1][0] / nw[1], acc[1][0] / nw[1] / chunks, acc[1][1] / nw[1], acc[1][1] / nw[1] / chunks, acc[1][2] / nw[1], acc[1][2] / nw[1] / chunks);
            fflush(stdout);
            *ms_out = 0.0;
            return;
        }
        const ConvTune tune = kind == BenchKind::Conv ? conv_tune_from_code(arg) : ConvTune{};
        auto run = [&] {
            switch (kind) {
            case BenchKind::Fused32: launch_wino_fused(p, dU, s, nullptr, arg); break;
            case BenchKind::Fused64T: launch_wino_fused64t(p, dU, s, arg); break;
            case BenchKind::Fused64: launch_wino_fused64(p, dU, s, arg); break;
            case BenchKind::Wino3:
                launch_wino_input(wp.in, s);
                launch_conv(wp.gemm, s);
                launch_wino_output(wp.out, s);
                break;
            case BenchKind::Wino3Gemm: launch_conv(wp.gemm, s); break;   // the f32 component GEMMs alone
            default: launch_conv(p, s, tune); break;
            }
        };
        for (int i = 0; i < 2; ++i) run();
        *ms_out = time_launches(s, iters, run);
    });
}

int irsde_debug_lpips_tap(irsde_engine* e, const float* in, int B, int H, int W, int normalize, int tap, float* dst, int64_t dims[4], void* stream) {
    return guard([&] {
        if (!e || !in || !dims) throw HipError("debug_lpips_tap: null argument");
        if (!lpips_engine(e)) throw HipError("debug_lpips_tap: not an LPIPS engine (irsde_create_lpips)");
        if (!e->finalized) throw HipError("debug_lpips_tap: weights not finalized");
        if (B < 1 || tap < 1 || tap > 5) throw HipError("debug_lpips_tap: B must be positive and tap in 1..5");
        const LpipsGeom g = lpips_geometry(H, W);
        dims[0] = B; dims[1] = g.h[tap - 1]; dims[2] = g.w[tap - 1]; dims[3] = kLpipsLayers[tap - 1].cout;
        if (!dst) return;
        std::lock_guard<std::mutex> lk(e->mu);
        DeviceScope dev_scope(e->cfg.device);
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        float* ws = lpips_workspace(e, B, H, W);
        float* taps[5];
        lpips_features(e->lpips, in, nullptr, B, H, W, normalize, ws, taps, s, nullptr);
        IRSDE_HIP_CHECK(hipMemcpyAsync(dst, taps[tap - 1], (size_t)dims[0] * dims[1] * dims[2] * dims[3] * sizeof(float), hipMemcpyDeviceToDevice, s));
        IRSDE_HIP_CHECK(hipStreamSynchronize(s));
    });
}

}  // extern "C"
