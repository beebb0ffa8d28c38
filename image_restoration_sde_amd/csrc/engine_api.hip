// libirsde_hip.so — the C ABI (include/irsde_hip.h) and the sampler loop.
//
// Host-side structure (all C++; PyTorch never appears here):
//   Engine      weights in kernel layout, FiLM/time table, coefficient table, plans
//   Plan        per (B,H,W): static activation arena + the launch list of ONE network evaluation
//               (ConditionalUNet.forward, DenoisingUNet_arch.py:85-134) built once, replayed T times
//   sample()    the reverse loop (sde_utils.py:252-299): [step_begin, prep, net, update] per t, either
//               eager or as one captured hipGraph replayed T times; the step index lives in device
//               memory (StepState) so the graph is t-invariant.
#include "engine.h"
#include <cmath>

using namespace irsde;

namespace irsde {
namespace {

thread_local std::string g_last_error;

hipEvent_t get_event(irsde_engine* e, size_t i) {
    while (e->ev_pool.size() <= i) {
        hipEvent_t ev;
        IRSDE_HIP_CHECK(hipEventCreate(&ev));
        e->ev_pool.push_back(ev);
    }
    return e->ev_pool[i];
}

void run_net(Plan* pl, hipStream_t s) {
    for (auto& op : pl->net_ops) op.fn(s);
}

UpdateParams make_update(irsde_engine* e, Plan* pl) {
    UpdateParams u{};
    u.x = pl->xin; u.mu = pl->cin; u.pred = pl->pred;
    const int64_t ps = pl->pred_stride;
    u.sb = (int64_t)pl->Hp * pl->Wp * ps; u.sc = 1; u.sy = (int64_t)pl->Wp * ps; u.sx = ps;
    u.st = step_of(e, pl); u.ctl = e->ctl;
    u.B = pl->B; u.C = e->cfg.in_nc; u.H = pl->H; u.W = pl->W;
    u.batch0 = pl->b0;
    return u;
}

// One reverse step of a plan on its stream, with the plan's (step state, FiLM row): the engine's for the slot-0 plans, its own for a sub-batch plan
void one_step(irsde_engine* e, Plan* pl, hipStream_t s) {
    launch_step_begin(step_of(e, pl), e->film_table, e->film_row, film_of(e, pl), e->coef_table, s);
    run_net(pl, s);
    launch_sde_update(make_update(e, pl), s);
}

// Captures one_step as the plan's step graph (once per plan: the step index lives in device memory, so the graph is t-invariant)
void ensure_step_graph(irsde_engine* e, Plan* pl, hipStream_t s) {
    if (pl->graph_exec) return;
    IRSDE_HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    try {
        one_step(e, pl, s);
    } catch (...) {
        hipGraph_t g = nullptr;
        (void)hipStreamEndCapture(s, &g);
        if (g) (void)hipGraphDestroy(g);
        throw;
    }
    IRSDE_HIP_CHECK(hipStreamEndCapture(s, &pl->graph));
    IRSDE_HIP_CHECK(hipGraphInstantiate(&pl->graph_exec, pl->graph, nullptr, nullptr, 0));
}

// r05: a batch split into concurrent sub-batches (nsub > 1 parts: plans of slot i + 1 holding images [b0, b0 + B / nsub) each).  Every part is a complete,
// independent sampler: its own step counter / coefficient row / FiLM row (Plan::own_step, own_film), its own captured step graph, its own stream (part 0: the engine stream,
// part i > 0: sub_stream[i - 1]) — the parts fork once behind the call's inputs (ev_fork) and join once in front of its outputs (ev_join); there is
// no per-step dependency between them, so the hardware queues overlap one part's per-image latency-bound kernels (naf_chain_kernel: one CU per image)
// with the other parts' bandwidth-bound ones.  (First version: fork / join INSIDE one captured step graph — the branches of a hipGraph replay did not
// overlap on ROCm 7.2: 156.9 -> 161.6 images/s on BASELINE configs[4].)  Nothing in a part depends on another part (no cross-batch op
// in the score network): the result is the un-split one up to the tilings the smaller plans choose.
void ensure_sub_streams(irsde_engine* e, int n) {
    if (!e->ev_fork) IRSDE_HIP_CHECK(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
    for (int i = 0; i + 1 < n; ++i) {
        if (!e->sub_stream[i]) IRSDE_HIP_CHECK(hipStreamCreateWithFlags(&e->sub_stream[i], hipStreamNonBlocking));
        if (!e->ev_join[i]) IRSDE_HIP_CHECK(hipEventCreateWithFlags(&e->ev_join[i], hipEventDisableTiming));
    }
}

// IRSDE_FLAG_FP16 = the 16-bit operand mode (IRSDE_FLAG_BF16's kernels, plans and weight copies) with IEEE fp16 rounding
void apply_fp16_flag(irsde_engine* e) {
    if (!(e->cfg.flags & IRSDE_FLAG_FP16)) return;
    if (e->cfg.flags & IRSDE_FLAG_BF16_ACT) {
        delete e;
        throw HipError("IRSDE_FLAG_FP16 keeps fp32 activation storage: it cannot be combined with IRSDE_FLAG_BF16_ACT");
    }
    e->cfg.flags |= IRSDE_FLAG_BF16;
}

}  // namespace

int guard(const std::function<void()>& f) {
    try {
        f();
        return IRSDE_OK;
    } catch (const HipError& ex) {
        g_last_error = ex.what();
        const std::string m = ex.what();
        if (m.find("weight") != std::string::npos) return IRSDE_ERR_WEIGHT;
        if (m.find(" failed: ") != std::string::npos) return IRSDE_ERR_HIP;
        return IRSDE_ERR_INVALID;
    } catch (const std::exception& ex) {
        g_last_error = ex.what();
        return IRSDE_ERR_INVALID;
    }
}

// The LPIPS tower's workspace for N images of H x W: kept in the engine, grown (after a device synchronisation) when a call needs more
float* lpips_workspace(irsde_engine* e, int N, int H, int W) {
    const size_t need = lpips_workspace_floats(N, H, W);
    if (e->lpips_ws_floats < need) {
        IRSDE_HIP_CHECK(hipDeviceSynchronize());
        if (e->lpips_ws) (void)hipFree(e->lpips_ws);
        e->lpips_ws = nullptr;
        e->lpips_ws_floats = 0;
        const hipError_t err = hipMalloc(&e->lpips_ws, need * sizeof(float));
        if (err == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            throw HipError("lpips: hipMalloc of " + std::to_string(need * sizeof(float)) + " bytes of workspace failed (out of memory): use a smaller batch");
        }
        IRSDE_HIP_CHECK(err);
        e->lpips_ws_floats = need;
    }
    return e->lpips_ws;
}

}  // namespace irsde

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

const char* irsde_last_error(void) { return g_last_error.c_str(); }
int irsde_version(void) { return 107; }  // changelog: include/irsde_hip.h

int irsde_create(const irsde_config* cfg, irsde_engine** out) {
    return guard([&] {
        if (!cfg || !out) throw HipError("null argument");
        if (cfg->nf % 32 || cfg->nf < 32) throw HipError("nf must be a positive multiple of 32");
        if (cfg->depth < 1 || cfg->depth > 6) throw HipError("depth out of range");
        if (cfg->in_nc < 1 || cfg->in_nc > 4 || cfg->out_nc < 1 || cfg->out_nc > 4)
            throw HipError("in_nc/out_nc must be in 1..4");
        if (cfg->in_nc != cfg->out_nc) throw HipError("sampler needs in_nc == out_nc");
        if ((cfg->nf << cfg->depth) > 2048) throw HipError("nf * 2^depth must be <= 2048");
        const bool stereo = (cfg->flags & IRSDE_FLAG_UNET_STEREO) != 0;
        if (stereo) {
            if (cfg->flags & (IRSDE_FLAG_BF16 | IRSDE_FLAG_BF16_ACT | IRSDE_FLAG_FP16 | IRSDE_FLAG_SPLIT_BF16X2 | IRSDE_FLAG_SPLIT_F16X2))
                throw HipError("IRSDE_FLAG_UNET_STEREO runs in fp32 only (the 16-bit and split-operand modes are not covered for the full-resolution SCAM network)");
            if (cfg->flags & IRSDE_FLAG_UNCOND_FULLATTN) throw HipError("IRSDE_FLAG_UNET_STEREO cannot be combined with IRSDE_FLAG_UNCOND_FULLATTN");
        }
        if ((cfg->flags & IRSDE_FLAG_SCAM_STREAM) && !stereo)
            throw HipError("IRSDE_FLAG_SCAM_STREAM: the stereo networks only (with IRSDE_FLAG_UNET_STEREO here, with IRSDE_FLAG_NAF_STEREO in irsde_create_nafnet)");
        if (cfg->flags & IRSDE_FLAG_F16_ACT) throw HipError("IRSDE_FLAG_F16_ACT: the image-space ConditionalNAFNet only (irsde_create_nafnet)");
        if (cfg->flags & IRSDE_FLAG_NAF_STEREO) throw HipError("IRSDE_FLAG_NAF_STEREO: the stereo network is a ConditionalNAFNet (irsde_create_nafnet)");
        if (cfg->flags & IRSDE_FLAG_NAF_UNCOND) throw HipError("IRSDE_FLAG_NAF_UNCOND: irsde_create_nafnet only (the unconditional UNet is IRSDE_FLAG_UNCOND_FULLATTN)");
        auto* e = new irsde_engine();
        e->cfg = *cfg;
        if (stereo) {   // the sampler state holds [L | R] per pair
            e->naf_ic = cfg->in_nc;
            e->cfg.in_nc = e->cfg.out_nc = 2 * cfg->in_nc;
        }
        if (cfg->flags & IRSDE_FLAG_BF16_ACT) {
            if (cfg->flags & IRSDE_FLAG_NAIVE_CONV) {
                delete e;
                throw HipError("IRSDE_FLAG_BF16_ACT: only the conditional UNet on the MFMA kernels stores bf16 activations");
            }
            e->cfg.flags |= IRSDE_FLAG_BF16;
        }
        apply_fp16_flag(e);
        e->time_dim = cfg->nf * 4;
        build_inventory(e);
        *out = e;
    });
}

int irsde_create_nafnet(const irsde_nafnet_config* cfg, irsde_engine** out) {
    return guard([&] {
        if (!cfg || !out) throw HipError("null argument");
        if (cfg->width % 32 || cfg->width < 32) throw HipError("width must be a positive multiple of 32");
        if (cfg->img_channel < 1 || cfg->img_channel > 8) throw HipError("img_channel must be in 1..8");
        if (cfg->n_enc < 1 || cfg->n_enc > 6 || cfg->n_dec != cfg->n_enc) throw HipError("need 1..6 encoder stages and as many decoder stages");
        if ((cfg->width << cfg->n_enc) > 2048) throw HipError("width * 2^stages must be <= 2048");
        if (cfg->flags & IRSDE_FLAG_F16_ACT) {   // fp16 activation storage: the image-space networks on the fp16 MFMA kernels
            const int f = cfg->flags;
            if (f & (IRSDE_FLAG_NAF_INTRO_SKIP | IRSDE_FLAG_NAF_LENS | IRSDE_FLAG_NAF_STEREO))
                throw HipError("IRSDE_FLAG_F16_ACT cannot be combined with IRSDE_FLAG_NAF_INTRO_SKIP / IRSDE_FLAG_NAF_LENS / IRSDE_FLAG_NAF_STEREO (the image-space "
                               "ConditionalNAFNet only: the latent networks' hot level is the per-image chain kernel)");
            if ((f & IRSDE_FLAG_BF16) && !(f & IRSDE_FLAG_FP16)) throw HipError("IRSDE_FLAG_F16_ACT implies IRSDE_FLAG_FP16: it cannot be combined with IRSDE_FLAG_BF16 alone");
            if (f & IRSDE_FLAG_BF16_ACT) throw HipError("IRSDE_FLAG_F16_ACT cannot be combined with IRSDE_FLAG_BF16_ACT (one storage type per engine)");
            if (f & (IRSDE_FLAG_SPLIT_BF16X2 | IRSDE_FLAG_SPLIT_F16X2))
                throw HipError("IRSDE_FLAG_F16_ACT cannot be combined with IRSDE_FLAG_SPLIT_BF16X2 / IRSDE_FLAG_SPLIT_F16X2 (split operands go with fp32 storage)");
            if (f & IRSDE_FLAG_NAIVE_CONV) throw HipError("IRSDE_FLAG_F16_ACT: only the MFMA kernels store fp16 activations (not IRSDE_FLAG_NAIVE_CONV)");
        }
        if (cfg->flags & IRSDE_FLAG_BF16_ACT) throw HipError("IRSDE_FLAG_BF16_ACT: conditional UNet only");
        if (cfg->flags & IRSDE_FLAG_UNET_STEREO) throw HipError("IRSDE_FLAG_UNET_STEREO: the stereo UNet is a ConditionalUNet (irsde_create)");
        const bool stereo = (cfg->flags & IRSDE_FLAG_NAF_STEREO) != 0;
        if ((cfg->flags & IRSDE_FLAG_SCAM_STREAM) && !stereo)
            throw HipError("IRSDE_FLAG_SCAM_STREAM: the stereo networks only (with IRSDE_FLAG_NAF_STEREO here, with IRSDE_FLAG_UNET_STEREO in irsde_create)");
        if (stereo) {
            if (cfg->flags & (IRSDE_FLAG_NAF_LENS | IRSDE_FLAG_NAF_INTRO_SKIP))
                throw HipError("IRSDE_FLAG_NAF_STEREO cannot be combined with IRSDE_FLAG_NAF_LENS / IRSDE_FLAG_NAF_INTRO_SKIP");
            if (cfg->img_channel > 4) throw HipError("IRSDE_FLAG_NAF_STEREO: img_channel must be in 1..4 (pairs of 2 img_channel channels)");
            if ((cfg->flags & (IRSDE_FLAG_SPLIT_BF16X2 | IRSDE_FLAG_SPLIT_F16X2)) || ((cfg->flags & IRSDE_FLAG_BF16) && !(cfg->flags & IRSDE_FLAG_FP16)))
                throw HipError("IRSDE_FLAG_NAF_STEREO runs in fp32 or with IRSDE_FLAG_FP16 only (the bf16 and split-operand modes are not covered for the SCAM network)");
        }
        if ((cfg->flags & IRSDE_FLAG_NAF_UNCOND) && (cfg->flags & (IRSDE_FLAG_NAF_STEREO | IRSDE_FLAG_NAF_LENS | IRSDE_FLAG_NAF_INTRO_SKIP)))
            throw HipError("IRSDE_FLAG_NAF_UNCOND cannot be combined with IRSDE_FLAG_NAF_STEREO / IRSDE_FLAG_NAF_LENS / IRSDE_FLAG_NAF_INTRO_SKIP");
        auto* e = new irsde_engine();
        e->arch = 1;
        e->naf_ic = cfg->img_channel;
        e->cfg.in_nc = e->cfg.out_nc = (stereo ? 2 : 1) * cfg->img_channel;   // stereo: the sampler state holds [L | R] per pair
        e->cfg.nf = cfg->width;
        e->cfg.depth = cfg->n_enc;  // pad multiple 2^stages (padder_size, DenoisingNAFNet_arch.py:147)
        e->cfg.device = cfg->device;
        e->cfg.flags = cfg->flags;
        if (e->cfg.flags & IRSDE_FLAG_F16_ACT) e->cfg.flags |= IRSDE_FLAG_FP16;
        apply_fp16_flag(e);
        e->time_dim = cfg->width * 4;
        for (int i = 0; i < cfg->n_enc; ++i) {
            if (cfg->enc_blk_nums[i] < 0 || cfg->dec_blk_nums[i] < 0) throw HipError("negative block count");
            e->naf_enc_nums.push_back(cfg->enc_blk_nums[i]);
            e->naf_dec_nums.push_back(cfg->dec_blk_nums[i]);
        }
        e->naf_mid_num = cfg->middle_blk_num;
        build_inventory_naf(e);
        *out = e;
    });
}

void irsde_destroy(irsde_engine* e) {
    if (!e) return;
    int prev_dev = -1;
    (void)hipGetDevice(&prev_dev);
    (void)hipSetDevice(e->cfg.device);
    (void)hipDeviceSynchronize();
    e->plans.clear();
    e->lat_plans.clear();
    for (auto ev : e->ev_pool) (void)hipEventDestroy(ev);
    if (e->ev_in) (void)hipEventDestroy(e->ev_in);
    if (e->ev_out) (void)hipEventDestroy(e->ev_out);
    if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
    for (auto ev : e->ev_join) if (ev) (void)hipEventDestroy(ev);
    for (auto st : e->sub_stream) if (st) (void)hipStreamDestroy(st);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    for (float* p : e->dev_allocs) (void)hipFree(p);
    for (auto& kv : e->bf16_copies) (void)hipFree(kv.second);
    if (e->coef_table) (void)hipFree(e->coef_table);
    if (e->film_table) (void)hipFree(e->film_table);
    if (e->lpips_ws) (void)hipFree(e->lpips_ws);
    if (e->lpips_partial) (void)hipFree(e->lpips_partial);
    if (prev_dev >= 0) (void)hipSetDevice(prev_dev);  // destroy runs from a Python finaliser: leave the current device alone
    delete e;
}

int irsde_num_weights(const irsde_engine* e) { return e ? (int)e->names.size() : 0; }
const char* irsde_weight_name(const irsde_engine* e, int i) {
    if (!e || i < 0 || i >= (int)e->names.size()) return nullptr;
    return e->names[i].c_str();
}
int irsde_weight_shape(const irsde_engine* e, int i, int64_t shape[4], int* ndim) {
    if (!e || i < 0 || i >= (int)e->names.size()) return IRSDE_ERR_INVALID;
    const auto& t = e->host.at(e->names[i]);
    *ndim = (int)t.shape.size();
    for (size_t k = 0; k < t.shape.size(); ++k) shape[k] = t.shape[k];
    return IRSDE_OK;
}

int irsde_load_weight(irsde_engine* e, const char* name, const float* data, const int64_t* shape, int ndim) {
    return guard([&] {
        if (!e || !name || !data) throw HipError("null argument");
        if (e->finalized) throw HipError("weights already finalized: create a new engine to reload weights");
        auto it = e->host.find(name);
        if (it == e->host.end()) throw HipError(std::string("unknown weight name: ") + name);
        HostTensor& t = it->second;
        size_t n = 1;
        bool same = ndim == (int)t.shape.size();
        for (int k = 0; k < ndim; ++k) {
            n *= (size_t)shape[k];
            if (same && shape[k] != t.shape[k]) same = false;
        }
        if (!same) throw HipError(std::string("weight shape mismatch for ") + name);
        t.data.assign(data, data + n);
        t.loaded = true;
    });
}

int irsde_finalize_weights(irsde_engine* e) {
    return guard([&] {
        if (!e) throw HipError("null engine");
        if (e->finalized) return;
        finalize(e);
    });
}

int irsde_set_schedule(irsde_engine* e, int T, const float* coef) {
    return guard([&] {
        if (!e || !coef || T < 1) throw HipError("bad schedule arguments");
        if (lpips_engine(e)) throw HipError("set_schedule: an LPIPS engine (irsde_create_lpips) has no schedule");
        if (!e->finalized) throw HipError("set_schedule: weights not finalized");
        DeviceScope dev_scope(e->cfg.device);
        IRSDE_HIP_CHECK(hipDeviceSynchronize());
        std::lock_guard<std::mutex> lk(e->mu);
        // captured graphs bake the table pointers into their kernel nodes: drop them with the old tables
        for (auto& pl : e->plans) {
            if (pl->graph_exec) (void)hipGraphExecDestroy(pl->graph_exec);
            if (pl->graph) (void)hipGraphDestroy(pl->graph);
            pl->graph_exec = nullptr;
            pl->graph = nullptr;
        }
        if (e->coef_table) (void)hipFree(e->coef_table);
        if (e->film_table) (void)hipFree(e->film_table);
        e->coef_table = e->film_table = nullptr;
        e->T = T;
        IRSDE_HIP_CHECK(hipMalloc(&e->coef_table, (size_t)(T + 1) * IRSDE_COEF_STRIDE * 4));
        IRSDE_HIP_CHECK(hipMemcpy(e->coef_table, coef, (size_t)(T + 1) * IRSDE_COEF_STRIDE * 4, hipMemcpyHostToDevice));
        IRSDE_HIP_CHECK(hipMalloc(&e->film_table, (size_t)(T + 1) * e->film_row * 4));
        std::vector<float> tv(T + 1);
        for (int t = 0; t <= T; ++t) tv[t] = (float)t;
        float* dtv = nullptr;
        IRSDE_HIP_CHECK(hipMalloc(&dtv, (T + 1) * sizeof(float)));
        IRSDE_HIP_CHECK(hipMemcpy(dtv, tv.data(), (T + 1) * sizeof(float), hipMemcpyHostToDevice));
        compute_film_rows(e, dtv, T + 1, e->film_table, e->stream);
        (void)hipFree(dtv);
    });
}

int irsde_unet_forward(irsde_engine* e, const float* xt, const float* cond, const int64_t* t_host, int nt, int B, int H,
                       int W, float* out, void* stream) {
    return guard([&] {
        const bool uncond_e = e && uncond_engine(e);
        if (!e || !xt || (!cond && !uncond_e) || !t_host || !out) throw HipError("null argument");
        if (!e->finalized) throw HipError("unet_forward: weights not finalized");
        if (nt != 1 && nt != B) throw HipError("unet_forward: need 1 or B timesteps");
        if (B < 1 || H < 2 || W < 2) throw HipError("unet_forward: bad shape");
        std::lock_guard<std::mutex> lk(e->mu);
        DeviceScope dev_scope(e->cfg.device);
        hipStream_t user = reinterpret_cast<hipStream_t>(stream);
        const bool per_sample = nt > 1;
        Plan* pl = get_plan(e, B, H, W, per_sample);
        hipStream_t s = e->stream;
        IRSDE_HIP_CHECK(hipEventRecord(e->ev_in, user));
        IRSDE_HIP_CHECK(hipStreamWaitEvent(s, e->ev_in, 0));
        const size_t img = (size_t)B * e->cfg.in_nc * H * W * sizeof(float);
        IRSDE_HIP_CHECK(hipMemcpyAsync(pl->xin, xt, img, hipMemcpyDeviceToDevice, s));
        if (cond) IRSDE_HIP_CHECK(hipMemcpyAsync(pl->cin, cond, img, hipMemcpyDeviceToDevice, s));
        const bool in_table = nt == 1 && e->film_table && t_host[0] >= 0 && t_host[0] <= e->T;
        if (in_table) {
            IRSDE_HIP_CHECK(hipMemcpyAsync(e->film_cur, e->film_table + (size_t)t_host[0] * e->film_row,
                                           (size_t)e->film_row * 4, hipMemcpyDeviceToDevice, s));
        } else {
            // stereo with per-pair times: one row per view v B + b (time = torch.cat([time, time], 0), stereo-sr DenoisingNAFNet_arch.py:213)
            const int rows = (stereo_engine(e) && nt > 1 ? 2 : 1) * nt;
            std::vector<float> tv(rows);
            for (int i = 0; i < rows; ++i) tv[i] = (float)t_host[i % nt];
            float* dtv = nullptr;
            IRSDE_HIP_CHECK(hipMalloc(&dtv, rows * sizeof(float)));
            IRSDE_HIP_CHECK(hipMemcpy(dtv, tv.data(), rows * sizeof(float), hipMemcpyHostToDevice));
            compute_film_rows(e, dtv, rows, e->film_cur, s);
            (void)hipFree(dtv);
        }
        run_net(pl, s);
        launch_unpack_pred(pl->pred, out, B, e->cfg.out_nc, H, W, pl->Hp, pl->Wp, pl->pred_stride, s);
        IRSDE_HIP_CHECK(hipEventRecord(e->ev_out, s));
        IRSDE_HIP_CHECK(hipStreamWaitEvent(user, e->ev_out, 0));
    });
}

int irsde_sample(irsde_engine* e, int mode, const float* xT, const float* mu, const float* noise, uint64_t seed,
                 uint64_t image_offset, int B, int H, int W, int T, int t_stop, float* out, void* stream,
                 int flags) {
    return guard([&] {
        if (!e || !xT || !out) throw HipError("null argument");
        if (!e->finalized || !e->film_table) throw HipError("sample: weights/schedule not set");
        if (mode < 0 || mode > 4) throw HipError("sample: bad mode");
        const bool uncond_e = uncond_engine(e);
        if ((mode >= 3) != uncond_e) throw HipError("sample: DenoisingSDE modes (3,4) go with the unconditional network and vice versa");
        if (!mu && !uncond_e) throw HipError("null argument");
        if (T < 0) T = e->T;
        if (T > e->T) throw HipError("sample: T exceeds the schedule length");
        if (B < 1 || H < 2 || W < 2) throw HipError("sample: bad shape");
        if (t_stop < 0 || (T > 0 && t_stop >= T) || (T == 0 && t_stop != 0)) throw HipError("sample: t_stop must be in [0, T)");
        const int nsteps = T - t_stop;
        std::lock_guard<std::mutex> lk(e->mu);
        DeviceScope dev_scope(e->cfg.device);
        hipStream_t user = reinterpret_cast<hipStream_t>(stream);
        if (T == 0) {
            // the reference's `for t in reversed(range(1, T + 1))` runs zero steps and returns the clone of xt
            // (e.g. reverse_ode(x, T=sde.get_optimal_timestep(sigma)) when the argmin is index 0)
            IRSDE_HIP_CHECK(hipMemcpyAsync(out, xT, (size_t)B * e->cfg.in_nc * H * W * 4, hipMemcpyDeviceToDevice, user));
            return;
        }
        hipStream_t s = e->stream;
        const bool profile = (flags & IRSDE_SAMPLE_PROFILE) != 0;
        const bool graph = (flags & IRSDE_SAMPLE_GRAPH) != 0 && !profile;
        const size_t img = (size_t)B * e->cfg.in_nc * H * W;
        // r06: a split NAFBlock-chain launch (naf_chain.hip, G work-groups per image) whose groups were not co-resident raised its error flag instead of
        // hanging the GPU: the results of that call were garbage — fail loudly at the next one (the call itself is asynchronous)
        for (auto& p : e->plans)
            for (const unsigned* f : p->chain_err) {
                unsigned v = 0;
                IRSDE_HIP_CHECK(hipMemcpy(&v, f, 4, hipMemcpyDeviceToHost));
                if (v) {
                    for (auto& sc : p->chain_scratch) naf_chain_split_reset(sc.first, sc.second);
                    char code[32];
                    snprintf(code, sizeof code, " [flag 0x%x]", v);
                    throw HipError(std::string("sample: the previous call's split NAFBlock-chain kernel timed out waiting for a work-group that was not resident (its results were invalid); "
                                               "set IRSDE_TUNING=1 IRSDE_NAF_CHAIN_SPLIT=1 if other work shares this GPU") + code);
                }
            }
        // The call runs as nsub >= 1 parts: part i is a plan of B / nsub images on its own stream (the slot-0 plan on the engine stream when nsub == 1)
        const int nsub = profile ? 1 : naf_subbatches(e, B, H, W);   // (the event-instrumented pass times the un-split plan: its kernels are the same)
        const int Bs = B / nsub;
        const size_t simg = img / nsub;
        struct Part { Plan* pl; hipStream_t st; };
        std::vector<Part> parts(nsub);
        auto part_plan = [&](int i) { return get_plan(e, Bs, H, W, false, nsub > 1 ? i + 1 : 0, i * Bs); };
        struct PartsScope { irsde_engine* e; PartsScope(irsde_engine* e_, int n) : e(e_) { e->plan_parts = n; } ~PartsScope() { e->plan_parts = 1; } } parts_scope(e, nsub);
        for (int i = 0; i < nsub; ++i) parts[i].pl = part_plan(i);
        for (int i = 0; i < nsub; ++i) (void)part_plan(i);   // (all parts most recently used: none of them is the next eviction victim)
        if (nsub > 1) ensure_sub_streams(e, nsub);
        for (int i = 0; i < nsub; ++i) parts[i].st = i == 0 ? s : e->sub_stream[i - 1];
        IRSDE_HIP_CHECK(hipEventRecord(e->ev_in, user));
        IRSDE_HIP_CHECK(hipStreamWaitEvent(s, e->ev_in, 0));
        launch_set_ctl(e->ctl, mode, noise, (long long)img, seed, image_offset, s);   // call-level arguments, shared by the parts (read-only during the call)
        if (nsub > 1) IRSDE_HIP_CHECK(hipEventRecord(e->ev_fork, s));
        for (int i = 0; i < nsub; ++i) {
            Plan* pl = parts[i].pl;
            hipStream_t t = parts[i].st;
            if (i > 0) IRSDE_HIP_CHECK(hipStreamWaitEvent(t, e->ev_fork, 0));
            IRSDE_HIP_CHECK(hipMemcpyAsync(pl->xin, xT + i * simg, simg * 4, hipMemcpyDeviceToDevice, t));
            if (mu) IRSDE_HIP_CHECK(hipMemcpyAsync(pl->cin, mu + i * simg, simg * 4, hipMemcpyDeviceToDevice, t));
            launch_set_step(step_of(e, pl), T, t);
            if (graph) ensure_step_graph(e, pl, t);
        }
        if (!profile) {
            // step-major launch order: the host feeds every part's queue in turn (a part-major order would enqueue T steps of part 0 before part 1 starts)
            for (int k = 0; k < nsteps; ++k)
                for (auto& p : parts) {
                    if (graph) IRSDE_HIP_CHECK(hipGraphLaunch(p.pl->graph_exec, p.st));
                    else one_step(e, p.pl, p.st);
                }
        } else {
            // eager with an event before every kernel group; interval k..k+1 belongs to group k
            Plan* pl = parts[0].pl;
            std::vector<int> kinds;
            size_t ei = 0;
            auto mark = [&](int kind) {
                IRSDE_HIP_CHECK(hipEventRecord(get_event(e, ei++), s));
                kinds.push_back(kind);
            };
            for (int i = 0; i < nsteps; ++i) {
                mark(OP_OTHER);
                launch_step_begin(step_of(e, pl), e->film_table, e->film_row, film_of(e, pl), e->coef_table, s);
                for (auto& op : pl->net_ops) {
                    mark(op.kind);
                    op.fn(s);
                }
                mark(OP_OTHER);
                launch_sde_update(make_update(e, pl), s);
            }
            IRSDE_HIP_CHECK(hipEventRecord(get_event(e, ei++), s));
            IRSDE_HIP_CHECK(hipStreamSynchronize(s));
            double ms[OP_NKINDS] = {0, 0, 0, 0, 0};
            const size_t per_step = pl->net_ops.size() + 2;
            e->op_ms.assign(pl->net_ops.size(), 0.0);
            e->op_desc.clear();
            for (auto& op : pl->net_ops) e->op_desc.push_back(op.desc);
            e->op_steps = nsteps;
            e->op_split = naf_subbatches(e, B, H, W);
            for (size_t k = 0; k < kinds.size(); ++k) {
                float t;
                IRSDE_HIP_CHECK(hipEventElapsedTime(&t, e->ev_pool[k], e->ev_pool[k + 1]));
                ms[kinds[k]] += t;
                const size_t in_step = k % per_step;
                if (in_step >= 1 && in_step <= pl->net_ops.size()) e->op_ms[in_step - 1] += t;
            }
            hipEvent_t e0 = e->ev_pool[0], e1 = e->ev_pool[kinds.size()];
            float wall;
            IRSDE_HIP_CHECK(hipEventElapsedTime(&wall, e0, e1));
            size_t nconv = 0;
            for (auto& op : pl->net_ops) nconv += op.kind == OP_CONV;
            e->profile[0] = ms[OP_CONV];
            e->profile[1] = pl->conv_flops * nsteps;
            e->profile[2] = (double)nconv * nsteps;
            e->profile[3] = pl->conv_bytes * nsteps;
            e->profile[4] = ms[OP_LN];
            e->profile[5] = ms[OP_ATTN];
            e->profile[6] = ms[OP_OTHER];
            e->profile[7] = wall;
            e->profile[8] = nsteps;
            e->profile[9] = ms[OP_WINO];
            e->profile[10] = pl->conv_exec_flops * nsteps;
            e->profile[11] = 0;
        }
        for (int i = 0; i < nsub; ++i) {
            IRSDE_HIP_CHECK(hipMemcpyAsync(out + i * simg, parts[i].pl->xin, simg * 4, hipMemcpyDeviceToDevice, parts[i].st));
            if (i > 0) {
                IRSDE_HIP_CHECK(hipEventRecord(e->ev_join[i - 1], parts[i].st));
                IRSDE_HIP_CHECK(hipStreamWaitEvent(s, e->ev_join[i - 1], 0));
            }
        }
        IRSDE_HIP_CHECK(hipEventRecord(e->ev_out, s));
        IRSDE_HIP_CHECK(hipStreamWaitEvent(user, e->ev_out, 0));
    });
}

int irsde_sde_step(int mode, int t, const float* coef_row, float* x, const float* mu, const float* eps_hat,
                   const float* noise_t, uint64_t seed, uint64_t image_offset, int B, int C, int H, int W,
                   void* stream) {
    return guard([&] {
        if (!coef_row || !x || !eps_hat || (!mu && mode < 3)) throw HipError("null argument");
        if (!mu) mu = x;  // DenoisingSDE has no mu term; the kernel still reads the pointer
        if (mode < 0 || mode > 4) throw HipError("sde_step: bad mode");
        UpdateParams u{};
        u.x = x; u.mu = mu; u.pred = eps_hat;
        u.sb = (int64_t)C * H * W; u.sc = (int64_t)H * W; u.sy = W; u.sx = 1;
        // noise_t is the draw for this step: index it with tstride 0
        u.noise = noise_t; u.noise_tstride = 0;
        u.st = nullptr; u.ctl = nullptr; u.t_imm = t;
        for (int i = 0; i < IRSDE_COEF_STRIDE; ++i) u.coef_imm[i] = coef_row[i];
        u.mode = mode; u.B = B; u.C = C; u.H = H; u.W = W; u.seed = seed; u.image_offset = image_offset;
        launch_sde_update(u, reinterpret_cast<hipStream_t>(stream));
    });
}

int irsde_philox_normal(float* out, int B, int CHW, int t, uint64_t seed, uint64_t image_offset, void* stream) {
    return guard([&] {
        if (!out) throw HipError("null argument");
        launch_philox_normal(out, B, CHW, t, seed, image_offset, reinterpret_cast<hipStream_t>(stream));
    });
}

int irsde_get_profile(const irsde_engine* e, double out[12]) {
    if (!e || !out) return IRSDE_ERR_INVALID;
    for (int i = 0; i < 12; ++i) out[i] = e->profile[i];
    return IRSDE_OK;
}

int irsde_debug_tap(irsde_engine* e, const char* name, float* dst, int64_t dims[4]) {
    return guard([&] {
        if (!e || !name || !dims) throw HipError("null argument");
        if (!(e->cfg.flags & IRSDE_FLAG_KEEP_ACTIVATIONS)) throw HipError("debug_tap needs IRSDE_FLAG_KEEP_ACTIVATIONS");
        Plan* pl = nullptr;
        for (auto& p : e->plans)
            if (!pl || p->last_use > pl->last_use) pl = p.get();
        if (!pl) throw HipError("debug_tap: no forward has run");
        auto it = pl->taps.find(name);
        if (it == pl->taps.end()) throw HipError(std::string("debug_tap: unknown tap ") + name);
        const Tensor& t = it->second;
        dims[0] = t.B; dims[1] = t.C; dims[2] = t.H; dims[3] = t.W;
        if (!dst) return;
        DeviceScope dev_scope(e->cfg.device);
        IRSDE_HIP_CHECK(hipDeviceSynchronize());
        float* tmp = nullptr;
        IRSDE_HIP_CHECK(hipMalloc(&tmp, t.numel() * 4));
        launch_nhwc_to_nchw(t.p, tmp, t.B, t.C, t.H, t.W, e->stream, t.bf16, t.f16);
        IRSDE_HIP_CHECK(hipStreamSynchronize(e->stream));
        IRSDE_HIP_CHECK(hipMemcpy(dst, tmp, t.numel() * 4, hipMemcpyDeviceToHost));
        (void)hipFree(tmp);
    });
}

int irsde_op_profile(irsde_engine* e, char* buf, int buflen) {
    return guard([&] {
        if (!e || !buf || buflen < 1) throw HipError("null argument");
        std::string out;
        char line[512];
        for (size_t i = 0; i < e->op_ms.size(); ++i) {
            snprintf(line, sizeof line, "%9.4f ms  %s\n", e->op_ms[i] / std::max(e->op_steps, 1), e->op_desc[i].c_str());
            out += line;
        }
        if (e->op_split > 1) {   // (label what was timed — parsers skip lines without the "ms" column)
            snprintf(line, sizeof line, "note: the un-split plan; irsde_sample runs this batch as %d concurrent sub-batches (own plans, streams, step graphs)\n", e->op_split);
            out += line;
        }
        strncpy(buf, out.c_str(), buflen - 1);
        buf[buflen - 1] = 0;
    });
}

int irsde_plan_describe(irsde_engine* e, int B, int H, int W, char* buf, int buflen) {
    return guard([&] {
        if (!e || !buf || buflen < 1) throw HipError("null argument");
        if (!e->finalized) throw HipError("plan_describe: weights not finalized");
        std::lock_guard<std::mutex> lk(e->mu);
        DeviceScope dev_scope(e->cfg.device);
        Plan* pl = get_plan(e, B, H, W, false);
        std::string out;
        for (auto& op : pl->net_ops) out += op.desc + "\n";
        const int nsub = naf_subbatches(e, B, H, W);
        if (nsub > 1) out += "note: the un-split plan; irsde_sample runs this batch as " + std::to_string(nsub) + " concurrent sub-batches of " + std::to_string(B / nsub) + " images (own plans)\n";
        strncpy(buf, out.c_str(), buflen - 1);
        buf[buflen - 1] = 0;
    });
}

int irsde_work_model(irsde_engine* e, int B, int H, int W, double out[2]) {
    return guard([&] {
        if (!e || !out) throw HipError("null argument");
        if (!e->finalized) throw HipError("work_model: weights not finalized");
        std::lock_guard<std::mutex> lk(e->mu);
        DeviceScope dev_scope(e->cfg.device);
        Plan* pl = get_plan(e, B, H, W, false);
        out[0] = pl->conv_flops;
        out[1] = pl->conv_bytes;
    });
}

int irsde_create_latent_unet(const irsde_latent_unet_config* cfg, irsde_engine** out) {
    return guard([&] {
        if (!cfg || !out) throw HipError("null argument");
        if (cfg->in_ch < 1 || cfg->in_ch > 32 || cfg->out_ch < 1 || cfg->out_ch > 4) throw HipError("in_ch must be in 1..32 and out_ch in 1..4");
        if (cfg->ch < 1 || cfg->n_mult < 1 || cfg->n_mult > 6) throw HipError("ch / ch_mult out of range");
        if (cfg->embed_dim < 1 || cfg->embed_dim > 32) throw HipError("embed_dim must be in 1..32");
        if (cfg->flags & IRSDE_FLAG_BF16_ACT) throw HipError("IRSDE_FLAG_BF16_ACT: conditional UNet only");
        if (cfg->flags & IRSDE_FLAG_F16_ACT) throw HipError("IRSDE_FLAG_F16_ACT: the image-space ConditionalNAFNet only (irsde_create_nafnet)");
        if (cfg->flags & IRSDE_FLAG_SCAM_STREAM) throw HipError("IRSDE_FLAG_SCAM_STREAM: the stereo networks only (irsde_create / irsde_create_nafnet)");
        auto* e = new irsde_engine();
        e->arch = 2;
        e->cfg.in_nc = cfg->in_ch; e->cfg.out_nc = cfg->out_ch; e->cfg.nf = cfg->ch; e->cfg.depth = cfg->n_mult;
        e->cfg.device = cfg->device; e->cfg.flags = cfg->flags;
        apply_fp16_flag(e);
        e->lat_in = cfg->in_ch; e->lat_out = cfg->out_ch; e->lat_ch = cfg->ch; e->lat_embed = cfg->embed_dim;
        for (int i = 0; i < cfg->n_mult; ++i) {
            if (cfg->ch_mult[i] < 1 || cfg->ch * cfg->ch_mult[i] > 2048) throw HipError("ch * ch_mult out of range");
            e->lat_mult.push_back(cfg->ch_mult[i]);
        }
        build_inventory_latent(e);
        *out = e;
    });
}

int irsde_latent_shapes(irsde_engine* e, int H, int W, int64_t latent_chw[3], int64_t* hidden_chw, int* n_hidden) {
    return guard([&] {
        if (!e || e->arch != 2 || !latent_chw || !n_hidden) throw HipError("latent_shapes: not a latent UNet engine / null argument");
        const int depth = (int)e->lat_mult.size(), sdiv = 1 << depth;
        const int Hp = (H + sdiv - 1) / sdiv * sdiv, Wp = (W + sdiv - 1) / sdiv * sdiv;
        latent_chw[0] = e->lat_embed; latent_chw[1] = Hp >> (depth - 1); latent_chw[2] = Wp >> (depth - 1);
        *n_hidden = 2 * depth + 1;
        if (hidden_chw) {
            auto dim = [&](int i) { return i == 0 ? e->lat_ch : e->lat_ch * e->lat_mult[i - 1]; };
            for (int k = 0; k < 2 * depth + 1; ++k) {
                const int lvl = k == 0 ? 0 : (k - 1) / 2;
                hidden_chw[3 * k] = dim(lvl); hidden_chw[3 * k + 1] = Hp >> lvl; hidden_chw[3 * k + 2] = Wp >> lvl;
            }
        }
    });
}

int irsde_latent_encode(irsde_engine* e, const float* x, int B, int H, int W, float* latent, float* const* hidden,
                        void* stream) {
    return guard([&] {
        if (!e || e->arch != 2 || !x || !latent) throw HipError("latent_encode: not a latent UNet engine / null argument");
        if (!e->finalized) throw HipError("latent_encode: weights not finalized");
        if (B < 1 || H < 2 || W < 2) throw HipError("latent_encode: bad shape");
        std::lock_guard<std::mutex> lk(e->mu);
        DeviceScope dev_scope(e->cfg.device);
        hipStream_t user = reinterpret_cast<hipStream_t>(stream), s = e->stream;
        LatentPlan* lp = get_latent_plan(e, B, H, W, false);
        Plan* pl = lp->plan.get();
        IRSDE_HIP_CHECK(hipEventRecord(e->ev_in, user));
        IRSDE_HIP_CHECK(hipStreamWaitEvent(s, e->ev_in, 0));
        launch_nchw_to_nhwc_pad(x, lp->image.p, B, e->lat_in, H, W, pl->Hp, pl->Wp, lp->image.C, 1, s);  // F.pad 'reflect'
        run_net(pl, s);
        const Tensor& L = lp->latent;
        launch_unpack_pred(L.p, latent, B, e->lat_embed, L.H, L.W, L.H, L.W, L.C, s);
        lp->resident = true;   // the skips stay in place for irsde_latent_decode(hidden = NULL) / irsde_latent_hidden
        for (size_t k = 0; hidden && k < lp->hidden.size(); ++k) {
            const Tensor& h = lp->hidden[k];
            if (!hidden[k]) throw HipError("latent_encode: null hidden pointer");
            launch_unpack_pred(h.p, hidden[k], B, lp->hidden_c[k], h.H, h.W, h.H, h.W, h.C, s);
        }
        IRSDE_HIP_CHECK(hipEventRecord(e->ev_out, s));
        IRSDE_HIP_CHECK(hipStreamWaitEvent(user, e->ev_out, 0));
    });
}

int irsde_latent_decode(irsde_engine* e, const float* latent, const float* const* hidden, int B, int H, int W, float* out,
                        void* stream) {
    return guard([&] {
        if (!e || e->arch != 2 || !latent || !out) throw HipError("latent_decode: not a latent UNet engine / null argument");
        if (!e->finalized) throw HipError("latent_decode: weights not finalized");
        std::lock_guard<std::mutex> lk(e->mu);
        DeviceScope dev_scope(e->cfg.device);
        hipStream_t user = reinterpret_cast<hipStream_t>(stream), s = e->stream;
        if (!hidden) {   // residency first: a call that is going to be refused must not build (or evict) any plan
            bool res = false;
            for (auto& q : e->lat_plans)
                if (!q->decode && q->plan->B == B && q->plan->H == H && q->plan->W == W) res = q->resident;
            if (!res) throw HipError("latent_decode: hidden == NULL needs a preceding irsde_latent_encode of the same B x H x W on this engine");
        }
        LatentPlan* lp = get_latent_plan(e, B, H, W, true);
        Plan* pl = lp->plan.get();
        LatentPlan* enc = get_latent_plan(e, B, H, W, false);   // (exists: the decode plan was built on it)
        if (hidden) enc->resident = false;   // the caller's skips overwrite the shared storage
        IRSDE_HIP_CHECK(hipEventRecord(e->ev_in, user));
        IRSDE_HIP_CHECK(hipStreamWaitEvent(s, e->ev_in, 0));
        const Tensor& L = lp->latent;
        launch_nchw_to_nhwc_pad(latent, L.p, B, e->lat_embed, L.H, L.W, L.H, L.W, L.C, 0, s);
        for (size_t k = 0; hidden && k < lp->hidden.size(); ++k) {
            const Tensor& h = lp->hidden[k];
            if (!hidden[k]) throw HipError("latent_decode: null hidden pointer");
            launch_nchw_to_nhwc_pad(hidden[k], h.p, B, lp->hidden_c[k], h.H, h.W, h.H, h.W, h.C, 0, s);
        }
        run_net(pl, s);
        launch_unpack_pred(lp->image.p, out, B, e->lat_out, H, W, pl->Hp, pl->Wp, 4, s);  // x[..., :H, :W]
        IRSDE_HIP_CHECK(hipEventRecord(e->ev_out, s));
        IRSDE_HIP_CHECK(hipStreamWaitEvent(user, e->ev_out, 0));
    });
}

int irsde_latent_hidden(irsde_engine* e, int B, int H, int W, int k, float* out, void* stream) {
    return guard([&] {
        if (!e || e->arch != 2 || !out) throw HipError("latent_hidden: not a latent UNet engine / null argument");
        std::lock_guard<std::mutex> lk(e->mu);
        DeviceScope dev_scope(e->cfg.device);
        hipStream_t user = reinterpret_cast<hipStream_t>(stream), s = e->stream;
        LatentPlan* enc = nullptr;
        for (auto& lp : e->lat_plans)
            if (!lp->decode && lp->plan->B == B && lp->plan->H == H && lp->plan->W == W) enc = lp.get();
        if (!enc || !enc->resident) throw HipError("latent_hidden: no resident skips of an irsde_latent_encode with this B x H x W");
        if (k < 0 || k >= (int)enc->hidden.size()) throw HipError("latent_hidden: bad skip index");
        IRSDE_HIP_CHECK(hipEventRecord(e->ev_in, user));
        IRSDE_HIP_CHECK(hipStreamWaitEvent(s, e->ev_in, 0));
        const Tensor& h = enc->hidden[k];
        launch_unpack_pred(h.p, out, B, enc->hidden_c[k], h.H, h.W, h.H, h.W, h.C, s);
        IRSDE_HIP_CHECK(hipEventRecord(e->ev_out, s));
        IRSDE_HIP_CHECK(hipStreamWaitEvent(user, e->ev_out, 0));
    });
}

int irsde_set_lens_info(irsde_engine* e, const float* info, int B) {
    return guard([&] {
        if (!e || !info || B < 1) throw HipError("null argument");
        if (e->arch != 1 || !naf_lens(e)) throw HipError("set_lens_info: not a latent-bokeh ConditionalNAFNet engine");
        if (!e->finalized) throw HipError("set_lens_info: weights not finalized");
        std::lock_guard<std::mutex> lk(e->mu);
        DeviceScope dev_scope(e->cfg.device);
        hipStream_t s = e->stream;
        if (e->cam_rows < B) {  // plans bake the table pointer: drop them when it moves
            IRSDE_HIP_CHECK(hipDeviceSynchronize());
            e->plans.clear();
            e->cam_cur = e->dmalloc((size_t)B * e->cam_row);
            e->cam_rows = B;
        }
        const int width = e->cfg.nf, td = e->time_dim;
        // cam_embed = cam_mlp(cat_i SinusoidalPosEmb(lens_info_i))  (:172-173); rows b*3+i of the sinusoid table are row b
        float *dv = nullptr, *emb = nullptr, *w1 = nullptr, *g1 = nullptr, *h2 = nullptr, *g2 = nullptr;
        IRSDE_HIP_CHECK(hipMalloc(&dv, (size_t)B * 3 * 4));
        IRSDE_HIP_CHECK(hipMemcpy(dv, info, (size_t)B * 3 * 4, hipMemcpyHostToDevice));
        IRSDE_HIP_CHECK(hipMalloc(&emb, (size_t)B * 3 * width * 4));
        IRSDE_HIP_CHECK(hipMalloc(&w1, (size_t)B * 2 * td * 4));
        IRSDE_HIP_CHECK(hipMalloc(&g1, (size_t)B * td * 4));
        IRSDE_HIP_CHECK(hipMalloc(&h2, (size_t)B * td * 4));
        IRSDE_HIP_CHECK(hipMalloc(&g2, (size_t)B * (td / 2) * 4));
        launch_sinusoid(dv, e->freqs, emb, B * 3, width / 2, s);
        launch_row_linear(emb, 3 * width, e->cm_w1, e->cm_b1, w1, 2 * td, B, 3 * width, 2 * td, ACT_NONE, ACT_NONE, s);
        launch_row_gate(w1, g1, B, td, s);
        launch_row_linear(g1, td, e->cm_w3, e->cm_b3, h2, td, B, td, td, ACT_NONE, ACT_NONE, s);
        launch_row_gate(h2, g2, B, td / 2, s);  // the block's cam_mlp starts with SimpleGate (:22-24)
        for (NafBlockW* b : e->naf_all)
            launch_row_linear(g2, td / 2, b->cam_w, b->cam_b, e->cam_cur + b->cam_off, e->cam_row, B, td / 2, 2 * b->c, ACT_NONE,
                              ACT_NONE, s);
        IRSDE_HIP_CHECK(hipStreamSynchronize(s));
        for (float* q : {dv, emb, w1, g1, h2, g2}) (void)hipFree(q);
        e->cam_set = B;
    });
}

int irsde_nafnet_set_local_pool(irsde_engine* e, int base_h, int base_w, int train_h, int train_w) {
    return guard([&] {
        if (!e) throw HipError("null argument");
        if (e->cfg.flags & IRSDE_FLAG_F16_ACT) throw HipError("set_local_pool: not with IRSDE_FLAG_F16_ACT (fp16 activation storage covers the image-space ConditionalNAFNet only)");
        if (e->arch != 1 || !(e->cfg.flags & IRSDE_FLAG_NAF_INTRO_SKIP))
            throw HipError("set_local_pool: CNAFNetLocal is the latent-task ConditionalNAFNet (irsde_create_nafnet with IRSDE_FLAG_NAF_INTRO_SKIP)");
        const int f = e->cfg.flags;
        if ((f & (IRSDE_FLAG_NAF_STEREO | IRSDE_FLAG_NAF_LENS | IRSDE_FLAG_NAF_UNCOND | IRSDE_FLAG_SPLIT_BF16X2 | IRSDE_FLAG_SPLIT_F16X2 | IRSDE_FLAG_BF16_ACT |
                  IRSDE_FLAG_NAIVE_CONV)) || ((f & IRSDE_FLAG_BF16) && !(f & IRSDE_FLAG_FP16)))
            throw HipError("set_local_pool: local pooling runs in fp32 or with IRSDE_FLAG_FP16 only, and not with IRSDE_FLAG_NAF_STEREO / _NAF_LENS / _NAF_UNCOND / "
                           "_NAIVE_CONV (not covered)");
        if (base_h < 1 || base_w < 1 || train_h < 1 || train_w < 1 || base_h > (1 << 20) || base_w > (1 << 20) || train_h > (1 << 20) || train_w > (1 << 20))
            throw HipError("set_local_pool: base and train sizes must be positive");
        std::lock_guard<std::mutex> lk(e->mu);
        const int old[4] = {e->tlsc_base_h, e->tlsc_base_w, e->tlsc_train_h, e->tlsc_train_w};
        e->tlsc_base_h = base_h; e->tlsc_base_w = base_w; e->tlsc_train_h = train_h; e->tlsc_train_w = train_w;
        int K0 = 0, K1 = 0;
        tlsc_window(e, e->cfg.depth, &K0, &K1);   // the smallest window (the middle blocks'): an empty one fails the reference's conversion forward
        if (K0 < 1 || K1 < 1) {
            e->tlsc_base_h = old[0]; e->tlsc_base_w = old[1]; e->tlsc_train_h = old[2]; e->tlsc_train_w = old[3];
            throw HipError("set_local_pool: the window of the deepest level is empty (train size too small for the network's depth)");
        }
        if (!e->plans.empty()) {   // plans bake the per-block choice: drop them
            DeviceScope dev_scope(e->cfg.device);
            IRSDE_HIP_CHECK(hipDeviceSynchronize());
            e->plans.clear();
        }
    });
}

int irsde_eval_metrics(const float* out, const float* gt, int B, int C, int H, int W, int crop_border, double* metrics,
                       void* stream) {
    return guard([&] {
        if (!out || !gt || !metrics || B < 1) throw HipError("null argument");
        std::vector<double> sums((size_t)B * 4);
        eval_metrics(out, gt, B, C, H, W, crop_border, sums.data(), reinterpret_cast<hipStream_t>(stream));
        const double Hc = H - 2 * crop_border, Wc = W - 2 * crop_border;
        const double n_rgb = Hc * Wc * C, n_y = Hc * Wc, v_rgb = (Hc - 10) * (Wc - 10) * C, v_y = (Hc - 10) * (Wc - 10);
        auto psnr = [](double sse, double n) {
            const double mse = sse / n;
            return mse == 0.0 ? INFINITY : 20.0 * log10(255.0 / sqrt(mse));
        };
        for (int b = 0; b < B; ++b) {
            metrics[b * 4 + 0] = psnr(sums[b * 4 + 0], n_rgb);
            metrics[b * 4 + 1] = sums[b * 4 + 1] / v_rgb;
            metrics[b * 4 + 2] = C == 3 ? psnr(sums[b * 4 + 2], n_y) : NAN;
            metrics[b * 4 + 3] = C == 3 ? sums[b * 4 + 3] / v_y : NAN;
        }
    });
}

int irsde_create_lpips(irsde_engine** out) {
    return guard([&] {
        if (!out) throw HipError("null argument");
        auto* e = new irsde_engine();
        e->arch = 3;
        build_inventory_lpips(e);
        *out = e;
    });
}

int irsde_lpips(irsde_engine* e, const float* in0, const float* in1, int B, int H, int W, int normalize, double* dist, double* terms, void* stream) {
    return guard([&] {
        if (!e || !in0 || !in1 || !dist) throw HipError("lpips: null argument");
        if (!lpips_engine(e)) throw HipError("lpips: not an LPIPS engine (irsde_create_lpips)");
        if (!e->finalized) throw HipError("lpips: weights not finalized");
        if (B < 1) throw HipError("lpips: B must be positive");
        const LpipsGeom g = lpips_geometry(H, W);   // throws below 31 x 31
        std::lock_guard<std::mutex> lk(e->mu);
        DeviceScope dev_scope(e->cfg.device);
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        float* ws = lpips_workspace(e, 2 * B, H, W);
        size_t np = 0;
        for (int l = 0; l < 5; ++l) np += (size_t)B * lpips_dist_blocks(g.h[l] * g.w[l]);
        if (e->lpips_partial_n < np) {
            IRSDE_HIP_CHECK(hipDeviceSynchronize());
            if (e->lpips_partial) (void)hipFree(e->lpips_partial);
            e->lpips_partial = nullptr;
            e->lpips_partial_n = 0;
            IRSDE_HIP_CHECK(hipMalloc(&e->lpips_partial, np * sizeof(double)));
            e->lpips_partial_n = np;
        }
        // an event in front of every launch group and one behind the last: the per-kernel times of this call (irsde_op_profile)
        std::vector<std::string> desc;
        auto mark = [&](const char* d) {
            IRSDE_HIP_CHECK(hipEventRecord(get_event(e, desc.size()), s));
            desc.push_back(d);
        };
        float* taps[5];
        lpips_features(e->lpips, in0, in1, B, H, W, normalize, ws, taps, s, mark);
        lpips_distances(e->lpips, taps, B, H, W, e->lpips_partial, s, mark);
        IRSDE_HIP_CHECK(hipEventRecord(get_event(e, desc.size()), s));
        std::vector<double> hp(np);
        IRSDE_HIP_CHECK(hipMemcpyAsync(hp.data(), e->lpips_partial, np * sizeof(double), hipMemcpyDeviceToHost, s));
        IRSDE_HIP_CHECK(hipStreamSynchronize(s));
        e->op_ms.assign(desc.size(), 0.0);
        e->op_desc = desc;
        e->op_steps = 1;
        for (size_t i = 0; i < desc.size(); ++i) {
            float ms = 0.f;
            IRSDE_HIP_CHECK(hipEventElapsedTime(&ms, e->ev_pool[i], e->ev_pool[i + 1]));
            e->op_ms[i] = ms;
        }
        size_t off = 0;
        for (int b = 0; b < B; ++b) dist[b] = 0.0;
        std::vector<double> tl((size_t)B * 5);
        for (int l = 0; l < 5; ++l) {
            const int hw = g.h[l] * g.w[l], nb = lpips_dist_blocks(hw);
            for (int b = 0; b < B; ++b) {
                double acc = 0.0;
                for (int k = 0; k < nb; ++k) acc += hp[off + (size_t)b * nb + k];
                tl[(size_t)b * 5 + l] = acc / hw;
            }
            off += (size_t)B * nb;
        }
        for (int b = 0; b < B; ++b) {
            double acc = 0.0;
            for (int l = 0; l < 5; ++l) {
                acc += tl[(size_t)b * 5 + l];
                if (terms) terms[(size_t)b * 5 + l] = tl[(size_t)b * 5 + l];
            }
            dist[b] = acc;
        }
    });
}

int irsde_tensor2img(const float* in, unsigned char* out, int B, int C, int H, int W, void* stream) {
    return guard([&] {
        if (!in || !out) throw HipError("null argument");
        tensor2img_u8(in, out, B, C, H, W, reinterpret_cast<hipStream_t>(stream));
    });
}

int irsde_upscale_bicubic(const float* in, float* out, int B, int C, int H, int W, int scale, void* stream) {
    return guard([&] {
        if (!in || !out) throw HipError("upscale_bicubic: null argument");
        if (B < 1 || C < 1 || H < 1 || W < 1) throw HipError("upscale_bicubic: B, C, H, W must be positive");
        if (scale < 1 || scale > 8) throw HipError("upscale_bicubic: scale must be an integer in 1..8");
        if ((int64_t)H * scale > INT32_MAX || (int64_t)W * scale > INT32_MAX) throw HipError("upscale_bicubic: output side beyond 2^31 - 1");
        upscale_bicubic(in, out, B, C, H, W, scale, reinterpret_cast<hipStream_t>(stream));
    });
}

int irsde_mask_to(const float* x, const unsigned char* masks, int Bm, int Hm, int Wm, int Cm, float* out, int B, int C, int H, int W,
                  void* stream) {
    return guard([&] {
        if (!x || !masks || !out) throw HipError("mask_to: null argument");
        if (B < 1 || C < 1 || H < 1 || W < 1 || Hm < 1 || Wm < 1) throw HipError("mask_to: B, C, H, W, Hm, Wm must be positive");
        if (Bm != 1 && Bm != B) throw HipError("mask_to: Bm must be 1 or B");
        if (Cm != 1 && Cm != C) throw HipError("mask_to: Cm must be 1 or C");
        mask_to(x, masks, Bm, Hm, Wm, Cm, out, B, C, H, W, reinterpret_cast<hipStream_t>(stream));
    });
}

int irsde_imresize(const float* in, float* out, int B, int C, int H, int W, int Ho, int Wo, const float* wH, const int* sH, int KH,
                   const float* wW, const int* sW, int KW, void* stream) {
    return guard([&] {
        if (!in || !out || !wH || !sH || !wW || !sW) throw HipError("imresize: null argument");
        if (B < 1 || C < 1 || H < 1 || W < 1 || Ho < 1 || Wo < 1) throw HipError("imresize: B, C, H, W, Ho, Wo must be positive");
        if (KH < 1 || KH > 32 || KW < 1 || KW > 32) throw HipError("imresize: KH and KW, the taps per output, must be in 1..32");
        if (H > (1 << 30) || W > (1 << 30)) throw HipError("imresize: input side beyond 2^30");
        imresize(in, out, B, C, H, W, Ho, Wo, wH, sH, KH, wW, sW, KW, reinterpret_cast<hipStream_t>(stream));
    });
}

}  // extern "C"
