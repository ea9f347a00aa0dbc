// Fused image entry points of the two hyperprior latent graphs (include/basic_hip.h section 8): the scale hyperprior, whose h_s
// gives a scale per latent, and the mean-scale hyperprior, whose h_s gives (scale, mean) and whose y is coded as round(y - mean).
//
// One C call = what GeneralCodec.compress / decompress (cbench/codecs/general_codec.py:44-130) run for the graph of
// configs/lossy_graph_scalable_exp_hp.py:182-215 through LatentGraphicalANSEntropyCoder.encode / decode
// (cbench/modules/entropy_coder/latent_graph.py:1232-1295): the same kernels of this library, in the same order as the
// module-by-module Python path launches them, so both paths give identical bytes.  Everything here is host
// orchestration: buffers, launches, two small synchronisations per compress (stream lengths, then the words).
#include "common.h"

#include <cstring>
#include <map>
#include <mutex>
#include <vector>

using namespace basic;

constexpr int kMaxTokenLanes = 4;


namespace {

struct DBuf {   // grow-only device buffer
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return BASIC_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = bytes + bytes / 4 + 256;
        BASIC_HIP_TRY(hipMalloc(&p, want));
        cap = want;
        return BASIC_OK;
    }
    template <class T> T *as() const { return static_cast<T *>(p); }
    ~DBuf() { if (p) (void)hipFree(p); }
};

struct HBuf {   // grow-only page-locked host buffer
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return BASIC_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = bytes + bytes / 2 + 4096;
        BASIC_HIP_TRY(hipHostMalloc(&p, want, hipHostMallocDefault));
        cap = want;
        return BASIC_OK;
    }
    template <class T> T *as() const { return static_cast<T *>(p); }
    ~HBuf() { if (p) (void)hipHostFree(p); }
};

// out[b][c][y][x] = in[b][c][y][x] for y < oh, x < ow  (prior[..., :h, :w].contiguous(), compressai_coder.py call sites)
__global__ void crop_planes_kernel(const float *__restrict__ in, int ih, int iw, float *__restrict__ out, int oh, int ow,
                                   int64_t planes)
{
    const int64_t total = planes * oh * ow;
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < total;
         i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int x = static_cast<int>(i % ow);
        const int y = static_cast<int>((i / ow) % oh);
        const int64_t pl = i / (static_cast<int64_t>(ow) * oh);
        out[i] = in[(pl * ih + y) * iw + x];
    }
}

// idx[b][c][hw] = c   (EntropyBottleneck indexes, compressai_coder.py:238-245 -> upstream _build_indexes)
__global__ void channel_index_kernel(int32_t *__restrict__ idx, int channels, int hw, int64_t total)
{
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < total;
         i += static_cast<int64_t>(gridDim.x) * blockDim.x)
        idx[i] = static_cast<int32_t>((i / hw) % channels);
}

// seg[i] = i * n (i <= streams); pos[i] = -1 (decoder: start from the stream head)
__global__ void seg_init_kernel(int64_t *__restrict__ seg, int64_t n, int streams, int64_t *__restrict__ pos)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= streams) seg[i] = static_cast<int64_t>(i) * n;
    if (pos && i < streams) pos[i] = -1;
}

// off[0] = 0, off[i + 1] = off[i] + max(nwords[i], 0)   (one wavefront; streams are few)
__global__ void offsets_kernel(const int32_t *__restrict__ nwords, int n, int64_t *__restrict__ off)
{
    const int lane = threadIdx.x;
    int64_t base = 0;
    if (lane == 0) off[0] = 0;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int i = c0 + lane;
        int64_t v = (i < n && nwords[i] > 0) ? nwords[i] : 0;
        for (int d = 1; d < 64; d <<= 1) {   // inclusive scan over the wave
            const int64_t up = __shfl_up(v, d, 64);
            if (lane >= d) v += up;
        }
        if (i < n) off[i + 1] = base + v;
        base += __shfl(v, 63, 64);
    }
}

int grid_for(int64_t total) { int64_t g = (total + 255) / 256; return static_cast<int>(g < 1 ? 1 : g > 4096 ? 4096 : g); }

}  // namespace

struct basic_hp_session {
    std::vector<const basic_conv_plan *> g_a, h_a, h_s, g_s;
    const basic_rans_tables *z_tables = nullptr, *y_tables = nullptr;
    int z_channels = 0, y_channels = 0, x_channels = 0, out_channels = 0, n_scales = 0;
    float scale_bound = 0.11f;
    // mean-scale graph: h_s ends in 2 * y_channels planes per image, scales [0, M) and means [M, 2 M) (upstream's chunk(2, 1)), and
    // y is coded as round(y - mean).  Both halves are read where h_s (or the crop) left them.
    bool mean_scale = false;
    int rans_waves = 0;
    int lanes = 1;       // y streams per image (basic_hp_session_set_stream_lanes)
    int res_lanes = 1;   // of the encoded batch held in h_words
    // quantiser step of the y latent (basic_hp_session_set_qsteps): empty = none, the step-less kernels.  Every call uploads
    // them on its own stream through h_steps; steps_done closes the last upload, the only reader of h_steps.
    std::vector<float> qsteps;
    HBuf h_steps;
    DBuf d_steps;
    hipEvent_t steps_done = nullptr;
    // rate targets (basic_hp_session_set_rate_targets): empty = none.  A call uploads budgets, first grid and the refinement's t
    // through h_rate (rate_up closes the upload), chooses the steps on the device into d_steps, and brings steps, predictions and
    // choice words back into h_rate_out beside the stream lengths (no synchronisation of its own).
    std::vector<int64_t> rate_budget;
    std::vector<float> rate_cand;
    int rate_passes = 0, rate_res_batch = 0;
    HBuf h_rate, h_rate_out;
    DBuf d_rate_in, d_rate_bits, d_rate_cand[2], d_rate_out;
    hipEvent_t rate_up = nullptr;
    // skip coding of the y latent (basic_hp_session_set_skip_rows): 0 = none, no extra launch.  Else the y streams are the compacted
    // ones: y_symc / y_idxc hold them back to back, seg_y their bounds as the compaction wrote them.
    int skip_rows = 0;
    DBuf skip_scratch, y_symc, y_idxc;
    DBuf d_medians, d_table;
    DBuf act[2], d_x, d_y, d_z, d_zhat, d_prior, d_scales;
    DBuf z_sym, z_idx, y_sym, y_idx, seg_z, seg_y, slots_z, slots_y, nw, off, packed, words, woff, state, pos;
    HBuf h_nw, h_words, h_in;
    std::vector<int64_t> off_z, off_y;   // word offsets of the last encoded batch (its words sit in h_words)
    int res_batch = 0, res_zh = 0, res_zw = 0, res_yh = 0, res_yw = 0;
    hipEvent_t in_done = nullptr;   // the last decode's upload out of h_in
    // Entropy side stream (only with the transform token, i.e. concurrent sessions): everything that is NOT a big
    // transform -- the hyper path's small kernels, both rANS stages, offsets / compaction / copies -- runs on a stream of
    // the highest priority, so that its few short workgroups are dispatched ahead of the thousands a transform of another
    // session has queued (measured: the hyper path took 3.0-3.7 ms beside another session's transforms, 0.7 ms alone).
    hipStream_t side = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    bool use_token = false;
    int token_lanes = 0;   // transform phases of all sessions admitted at a time (0 = no ordering)
    hipEvent_t enc_phase = nullptr, dec_phase = nullptr;   // close this session's transform phases (see TransformToken)
    // Upload of a host-resident batch (general_codec.py:46-47): on its own stream, ordered only after the PREVIOUS call's
    // analysis transform (the last reader of d_x), so it runs beside whatever the caller's stream still has queued (the
    // previous decode's chains and synthesis transform) instead of between that and this call's first layer.
    hipStream_t copy = nullptr;
    hipEvent_t x_free = nullptr, x_ready = nullptr;
    bool x_read_pending = false;
    // 8-bit images (basic_hp_*_images_u8): a uint8 batch is staged in u8_in and converted into d_x, a reconstruction is decoded
    // into d_xhat and converted out of it (into u8_out when the caller's buffer is host memory).  u8_free: the last conversion
    // out of u8_in; xhat_free: the last conversion out of d_xhat.  Either may have run on another stream than the next call's.
    DBuf u8_in, u8_out, d_xhat;
    hipEvent_t u8_free = nullptr, xhat_free = nullptr;
    bool u8_read_pending = false, xhat_read_pending = false;
    ~basic_hp_session();
};

namespace {

// runs a chain of layer plans; the result lands in *out_buf (a session buffer) -- or in d_final when given
int run_chain(basic_hp_session *s, const std::vector<const basic_conv_plan *> &plans, const float *d_in, int batch, int h, int w,
              DBuf *out_buf, float *d_final, int *oh_out, int *ow_out, hipStream_t st)
{
    const float *cur = d_in;
    int flip = 0;
    for (size_t i = 0; i < plans.size(); ++i) {
        int oh = 0, ow = 0, co = 0;
        int rc = basic_conv_plan_out_hw(plans[i], h, w, &oh, &ow);
        if (rc) return rc;
        rc = basic_conv_plan_channels(plans[i], nullptr, &co);
        if (rc) return rc;
        const size_t bytes = sizeof(float) * static_cast<size_t>(batch) * co * oh * ow;
        float *dst;
        if (i + 1 == plans.size()) {
            if (d_final) dst = d_final;
            else { rc = out_buf->ensure(bytes); if (rc) return rc; dst = out_buf->as<float>(); }
        } else {
            rc = s->act[flip].ensure(bytes);
            if (rc) return rc;
            dst = s->act[flip].as<float>();
            flip ^= 1;
        }
        rc = basic_conv_forward_dev(plans[i], cur, batch, h, w, dst, st);
        if (rc) return rc;
        cur = dst;
        h = oh;
        w = ow;
    }
    if (oh_out) *oh_out = h;
    if (ow_out) *ow_out = w;
    return BASIC_OK;
}

int chain_out_hw(const std::vector<const basic_conv_plan *> &plans, int h, int w, int *oh, int *ow)
{
    for (const auto *p : plans) {
        int a = 0, b = 0;
        int rc = basic_conv_plan_out_hw(p, h, w, &a, &b);
        if (rc) return rc;
        h = a;
        w = b;
    }
    *oh = h;
    *ow = w;
    return BASIC_OK;
}

// The "transform token": sessions that opt in (basic_hp_session_set_transform_token) run their MFMA-heavy phases one
// after another in GPU time, in the order their host threads enqueue them -- a phase starts with a stream-wait on the
// event that closed the previous holder's phase and ends by recording its own.  Without it, equal workers drift into
// lock-step (all in their transforms together, sharing the chip; then all in their rANS chains together, leaving it
// idle); with it, one worker's chains always run beside another worker's transforms.  Nothing blocks on the host
// except the short critical section that keeps wait / launches / record of one phase together.
struct TransformToken {
    std::mutex mu;
    // per device: the events that close the most recently enqueued phases, one per LANE (owned by the sessions that recorded
    // them).  A new phase waits for the phase that used its lane last, so `lanes` phases run side by side: 1 = strictly one
    // after another (full batches fill the chip on their own), 2 = two at a time (small batches: one session's launches
    // leave compute units idle and tile counts quantise badly, two sessions' launches interleave)
    struct Dev {
        hipEvent_t lane[kMaxTokenLanes] = {};
        int cursor = 0;
    };
    std::map<int, Dev> dev;
};
TransformToken g_token;

struct TokenPhase {   // RAII: a phase of one session on one stream
    basic_hp_session *s;
    hipStream_t st;
    hipEvent_t *evt;
    bool on;
    TransformToken::Dev *dev = nullptr;
    int slot = 0;
    int rc = BASIC_OK;
    TokenPhase(basic_hp_session *s_, hipStream_t st_, hipEvent_t *evt_);
    int close();
    ~TokenPhase() { if (on) (void)close(); }
};

struct WavesGuard {   // the session's rANS geometry / tile hand-out apply to this thread's launches for the duration of a call
    int prev;
    bool prev_dyn;
    explicit WavesGuard(int w, bool concurrent = false) : prev(set_rans_waves(w)), prev_dyn(set_dynamic_tiles(concurrent)) {}
    ~WavesGuard() { set_rans_waves(prev); set_dynamic_tiles(prev_dyn); }
};

// the stream the non-transform work of a call goes to: the caller's, or (token mode) the session's priority stream,
// ordered after everything enqueued on the caller's stream so far
int entropy_stream(basic_hp_session *s, hipStream_t st, hipStream_t *out)
{
    *out = st;
    if (!s->use_token) return BASIC_OK;
    if (!s->side) {
        int lo = 0, hi = 0;   // numerically lowest = greatest priority
        BASIC_HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
        BASIC_HIP_TRY(hipStreamCreateWithPriority(&s->side, hipStreamNonBlocking, hi));
        BASIC_HIP_TRY(hipEventCreateWithFlags(&s->fork, hipEventDisableTiming));
        BASIC_HIP_TRY(hipEventCreateWithFlags(&s->join, hipEventDisableTiming));
    }
    BASIC_HIP_TRY(hipEventRecord(s->fork, st));
    BASIC_HIP_TRY(hipStreamWaitEvent(s->side, s->fork, 0));
    *out = s->side;
    return BASIC_OK;
}

// the caller's stream continues after the side stream's work
int rejoin(basic_hp_session *s, hipStream_t st, hipStream_t es)
{
    if (es == st) return BASIC_OK;
    BASIC_HIP_TRY(hipEventRecord(s->join, es));
    BASIC_HIP_TRY(hipStreamWaitEvent(st, s->join, 0));
    return BASIC_OK;
}

TokenPhase::TokenPhase(basic_hp_session *s_, hipStream_t st_, hipEvent_t *evt_) : s(s_), st(st_), evt(evt_), on(s_->token_lanes > 0)
{
    if (!on) return;
    g_token.mu.lock();
    int d = 0;
    hipError_t e = hipGetDevice(&d);
    if (e == hipSuccess && !*evt) e = hipEventCreateWithFlags(evt, hipEventDisableTiming);
    if (e == hipSuccess) {
        dev = &g_token.dev[d];
        slot = dev->cursor % s->token_lanes;
        hipEvent_t prev = dev->lane[slot];
        if (prev && prev != *evt) e = hipStreamWaitEvent(st, prev, 0);
    }
    if (e != hipSuccess) rc = hip_fail(e, "transform token: wait", __FILE__, __LINE__);
}

int TokenPhase::close()
{
    if (!on) return rc;
    on = false;
    hipError_t e = hipEventRecord(*evt, st);
    if (e == hipSuccess && dev) {
        dev->lane[slot] = *evt;
        dev->cursor = (slot + 1) % s->token_lanes;
    }
    g_token.mu.unlock();
    if (e != hipSuccess && rc == BASIC_OK) rc = hip_fail(e, "transform token: record", __FILE__, __LINE__);
    return rc;
}

}  // namespace

extern "C" int basic_hp_session_set_transform_token(basic_hp_session *s, int enable)
{
    BASIC_REQUIRE(s && enable >= 0 && enable <= kMaxTokenLanes, "hp_session_set_transform_token: 0 (off) or 1 .. 4 phases at a time");
    s->token_lanes = enable;
    s->use_token = enable != 0;
    return BASIC_OK;
}

extern "C" int basic_hp_session_create(const basic_conv_plan *const *g_a, int n_g_a, const basic_conv_plan *const *h_a, int n_h_a,
                                       const basic_conv_plan *const *h_s, int n_h_s, const basic_conv_plan *const *g_s, int n_g_s,
                                       const float *eb_medians, int z_channels, const basic_rans_tables *z_tables,
                                       const float *scale_table, int n_scales, float scale_bound,
                                       const basic_rans_tables *y_tables, basic_hp_session **out)
{
    int rc = require_device();
    if (rc) return rc;
    BASIC_REQUIRE(g_a && h_a && h_s && g_s && n_g_a >= 1 && n_h_a >= 1 && n_h_s >= 1 && n_g_s >= 1 && eb_medians && z_tables &&
                      scale_table && n_scales >= 2 && y_tables && out && z_channels >= 1,
                  "hp_session_create: bad argument");
    auto *s = new basic_hp_session();
    s->g_a.assign(g_a, g_a + n_g_a);
    s->h_a.assign(h_a, h_a + n_h_a);
    s->h_s.assign(h_s, h_s + n_h_s);
    s->g_s.assign(g_s, g_s + n_g_s);
    for (auto *list : {&s->g_a, &s->h_a, &s->h_s, &s->g_s})
        for (const auto *p : *list)
            if (!p) { delete s; set_error("hp_session_create: null layer plan"); return BASIC_ERR_INVALID; }
    int ci = 0, co = 0;
    basic_conv_plan_channels(s->g_a.front(), &s->x_channels, nullptr);
    basic_conv_plan_channels(s->g_a.back(), nullptr, &s->y_channels);
    basic_conv_plan_channels(s->h_a.front(), &ci, nullptr);
    basic_conv_plan_channels(s->h_a.back(), nullptr, &co);
    bool ok = ci == s->y_channels && co == z_channels;
    basic_conv_plan_channels(s->h_s.front(), &ci, nullptr);
    basic_conv_plan_channels(s->h_s.back(), nullptr, &co);
    // y_channels outputs: scales only, the GaussianConditional graph; 2 * y_channels: (scales, means), the mean-scale graph
    s->mean_scale = co == 2 * s->y_channels;
    ok = ok && ci == z_channels && (co == s->y_channels || s->mean_scale);
    basic_conv_plan_channels(s->g_s.front(), &ci, nullptr);
    basic_conv_plan_channels(s->g_s.back(), nullptr, &s->out_channels);
    ok = ok && ci == s->y_channels;
    if (!ok) {
        delete s;
        set_error("hp_session_create: channel counts of the transforms do not chain (x->y->z->scales(y) or (scales, means)(y)->x)");
        return BASIC_ERR_INVALID;
    }
    s->z_channels = z_channels;
    s->z_tables = z_tables;
    s->y_tables = y_tables;
    s->n_scales = n_scales;
    s->scale_bound = scale_bound;
    rc = s->d_medians.ensure(sizeof(float) * z_channels);
    if (!rc) rc = s->d_table.ensure(sizeof(float) * n_scales);
    if (rc) { delete s; return rc; }
    hipError_t e = hipMemcpy(s->d_medians.p, eb_medians, sizeof(float) * z_channels, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s->d_table.p, scale_table, sizeof(float) * n_scales, hipMemcpyHostToDevice);
    if (e != hipSuccess) { delete s; return hip_fail(e, "hp_session_create upload", __FILE__, __LINE__); }
    *out = s;
    return BASIC_OK;
}

basic_hp_session::~basic_hp_session()
{
    {
        std::lock_guard<std::mutex> lock(g_token.mu);
        for (auto &kv : g_token.dev)
            for (hipEvent_t &e : kv.second.lane)
                if (e && (e == enc_phase || e == dec_phase)) {
                    (void)hipEventSynchronize(e);   // whoever waits on it has been released
                    e = nullptr;
                }
    }
    for (hipEvent_t e : {in_done, enc_phase, dec_phase, fork, join, x_free, x_ready, u8_free, xhat_free, steps_done, rate_up})
        if (e) (void)hipEventDestroy(e);
    if (side) (void)hipStreamDestroy(side);
    if (copy) (void)hipStreamDestroy(copy);
}

extern "C" void basic_hp_session_destroy(basic_hp_session *s) { delete s; }

extern "C" int basic_hp_session_set_rans_waves(basic_hp_session *s, int waves_per_block)
{
    BASIC_REQUIRE(s && (waves_per_block == 0 || waves_per_block == 1 || waves_per_block == 2 || waves_per_block == 4 ||
                        waves_per_block == 8 || waves_per_block == 16),
                  "hp_session_set_rans_waves: 0, 1, 2, 4, 8 or 16");
    s->rans_waves = waves_per_block;
    return BASIC_OK;
}

extern "C" int basic_hp_session_set_stream_lanes(basic_hp_session *s, int lanes)
{
    BASIC_REQUIRE(s && lanes >= 1 && lanes <= 256, "hp_session_set_stream_lanes: an integer in [1, 256]");
    s->lanes = lanes;
    s->res_batch = 0;   // a held batch was framed for the previous lane count
    return BASIC_OK;
}

extern "C" int basic_hp_session_set_qsteps(basic_hp_session *s, const float *host_steps, int n)
{
    BASIC_REQUIRE(s && n >= 0 && (n == 0 || host_steps), "hp_session_set_qsteps: bad argument");
    BASIC_REQUIRE(n == 0 || s->rate_budget.empty(), "hp_session_set_qsteps: rate targets are set -- clear them first (one way to state the step at a time)");
    for (int i = 0; i < n; ++i)   // NaN fails both comparisons' conjunction, infinities the upper one
        BASIC_REQUIRE(host_steps[i] >= BASIC_QSTEP_MIN && host_steps[i] <= BASIC_QSTEP_MAX,
                      "hp_session_set_qsteps: every step must be finite and in [2^-4, 2^6]");
    s->qsteps.assign(host_steps, host_steps + n);
    s->res_batch = 0;   // a held batch was coded with the previous steps
    return BASIC_OK;
}

extern "C" int basic_hp_session_set_rate_targets(basic_hp_session *s, const int64_t *host_budget_bytes, int n, const float *host_cand,
                                                 int n_cand, int passes)
{
    BASIC_REQUIRE(s && n >= 0, "hp_session_set_rate_targets: bad argument");
    if (n == 0) {
        s->rate_budget.clear();
        s->rate_cand.clear();
        s->rate_passes = 0;
        s->res_batch = 0;
        return BASIC_OK;
    }
    BASIC_REQUIRE(host_budget_bytes && host_cand, "hp_session_set_rate_targets: bad argument");
    BASIC_REQUIRE(s->skip_rows == 0, "hp_session_set_rate_targets: skip rows are set -- the rate curve would count symbols that are not coded");
    BASIC_REQUIRE(s->qsteps.empty(), "hp_session_set_rate_targets: quantiser steps are set -- clear them first (one way to state the step at a time)");
    BASIC_REQUIRE(n_cand >= 2 && n_cand <= 32 && passes >= 1 && passes <= 3, "hp_session_set_rate_targets: 2 to 32 candidates, 1 to 3 passes");
    for (int i = 0; i < n; ++i) BASIC_REQUIRE(host_budget_bytes[i] >= 1, "hp_session_set_rate_targets: every budget must be at least one byte");
    for (int k = 0; k < n_cand; ++k)   // NaN fails the conjunction
        BASIC_REQUIRE(host_cand[k] >= BASIC_QSTEP_MIN && host_cand[k] <= BASIC_QSTEP_MAX && (k == 0 || host_cand[k] > host_cand[k - 1]),
                      "hp_session_set_rate_targets: candidates must be strictly ascending and in [2^-4, 2^6]");
    s->rate_budget.assign(host_budget_bytes, host_budget_bytes + n);
    s->rate_cand.assign(host_cand, host_cand + n_cand);
    s->rate_passes = passes;
    s->res_batch = 0;   // a held batch was coded under the previous targets
    return BASIC_OK;
}

extern "C" int basic_hp_session_set_skip_rows(basic_hp_session *s, int rows)
{
    BASIC_REQUIRE(s && rows >= 0 && rows <= s->n_scales, "hp_session_set_skip_rows: an integer in [0, rows of the scale table]");
    BASIC_REQUIRE(rows == 0 || s->rate_budget.empty(),
                  "hp_session_set_skip_rows: rate targets are set -- the rate curve would count symbols that are not coded");
    s->skip_rows = rows;
    s->res_batch = 0;   // a held batch was coded under the previous rule
    return BASIC_OK;
}

extern "C" int basic_hp_session_rate_result(const basic_hp_session *s, float *steps, int64_t *pred_bytes, int32_t *flags, int n)
{
    BASIC_REQUIRE(s && n >= 1, "hp_session_rate_result: bad argument");
    BASIC_REQUIRE(s->rate_res_batch == n, "hp_session_rate_result: the session's last call coded no rate-controlled batch of n images");
    const char *p = static_cast<const char *>(s->h_rate_out.p);   // int64 pred [n] | float steps [n] | int32 choice [n]
    if (pred_bytes) std::memcpy(pred_bytes, p, sizeof(int64_t) * n);
    if (steps) std::memcpy(steps, p + sizeof(int64_t) * n, sizeof(float) * n);
    if (flags) std::memcpy(flags, p + (sizeof(int64_t) + sizeof(float)) * n, sizeof(int32_t) * n);
    return BASIC_OK;
}

extern "C" int64_t basic_hp_encode_bound(const basic_hp_session *s, int batch, int h, int w)
{
    if (!s || batch < 1 || h < 1 || w < 1) return -1;
    int yh, yw, zh, zw;
    if (chain_out_hw(s->g_a, h, w, &yh, &yw) || chain_out_hw(s->h_a, yh, yw, &zh, &zw)) return -1;
    const int64_t ny = static_cast<int64_t>(s->y_channels) * yh * yw, nz = static_cast<int64_t>(s->z_channels) * zh * zw;
    // worst case of the coder: 3 n + 4 words per stream (the retry slot of the bypass-heavy case); y: lanes streams per image
    const int64_t K = s->lanes;
    return 4 + (12 + 4ll * batch) + (12 + 4ll * batch * K) + 4ll * batch * ((3 * ny + 4 * K) + (3 * nz + 4));
}

namespace {

// the session's steps serve a call of `batch` images: one each, or one for all
bool qsteps_fit(const basic_hp_session *s, int batch)
{
    return s->qsteps.empty() || s->qsteps.size() == 1 || s->qsteps.size() == static_cast<size_t>(batch);
}

// the same for the session's byte budgets
bool budgets_fit(const basic_hp_session *s, int batch)
{
    return s->rate_budget.empty() || s->rate_budget.size() == 1 || s->rate_budget.size() == static_cast<size_t>(batch);
}

// Rate control of a call: the steps of its `batch` images into d_steps, chosen on the device from the curves of the y latent
// (sy = batch * lanes streams of nyl symbols) under the budgets, the z streams' word counts (d_nw_z, written earlier on `st`)
// counted in.  Enqueues only; the results travel to h_rate_out for the caller's next synchronisation of `st`.
int choose_steps(basic_hp_session *s, const float *d_y, const float *d_scales, const float *d_means, int64_t param_stride, int batch,
                 int lanes, int64_t nyl, const int32_t *d_nw_z, hipStream_t st)
{
    const int K = static_cast<int>(s->rate_cand.size());
    const int sy = batch * lanes;
    // upload: int64 budget [batch] | float cand [K] | float t [K]
    const size_t in_bytes = sizeof(int64_t) * batch + 2 * sizeof(float) * K;
    if (s->rate_up) BASIC_HIP_TRY(hipEventSynchronize(s->rate_up));   // the previous upload has left h_rate
    else BASIC_HIP_TRY(hipEventCreateWithFlags(&s->rate_up, hipEventDisableTiming));
    const size_t out_bytes = (sizeof(int64_t) + sizeof(float) + sizeof(int32_t)) * batch;
    int rc = s->h_rate.ensure(in_bytes);
    if (!rc) rc = s->d_rate_in.ensure(in_bytes);
    if (!rc) rc = s->d_rate_bits.ensure(sizeof(uint64_t) * static_cast<size_t>(sy) * K);
    if (!rc) rc = s->d_rate_cand[0].ensure(sizeof(float) * static_cast<size_t>(batch) * K);
    if (!rc) rc = s->d_rate_cand[1].ensure(sizeof(float) * static_cast<size_t>(batch) * K);
    if (!rc) rc = s->d_rate_out.ensure(out_bytes);
    if (!rc) rc = s->h_rate_out.ensure(out_bytes);
    if (!rc) rc = s->d_steps.ensure(sizeof(float) * batch);
    if (rc) return rc;
    int64_t *h_budget = s->h_rate.as<int64_t>();
    for (int b = 0; b < batch; ++b) h_budget[b] = s->rate_budget[s->rate_budget.size() == 1 ? 0 : b];
    float *h_cand = reinterpret_cast<float *>(h_budget + batch), *h_t = h_cand + K;
    for (int k = 0; k < K; ++k) {
        h_cand[k] = s->rate_cand[k];
        h_t[k] = static_cast<float>(k + 1) / static_cast<float>(K);
    }
    BASIC_HIP_TRY(hipMemcpyAsync(s->d_rate_in.p, s->h_rate.p, in_bytes, hipMemcpyHostToDevice, st));
    BASIC_HIP_TRY(hipEventRecord(s->rate_up, st));
    const int64_t *d_budget = s->d_rate_in.as<int64_t>();
    const float *d_cand = reinterpret_cast<const float *>(d_budget + batch), *d_t = d_cand + K;
    int64_t *d_pred = s->d_rate_out.as<int64_t>();
    float *d_steps_res = reinterpret_cast<float *>(d_pred + batch);
    int32_t *d_choice = reinterpret_cast<int32_t *>(d_steps_res + batch);
    int per_image = 0;
    for (int pass = 0; pass < s->rate_passes; ++pass) {
        if (pass > 0) {
            float *next = s->d_rate_cand[pass & 1].as<float>();
            rc = basic_rate_refine_dev(d_cand, per_image, K, d_choice, batch, d_t, next, st);
            if (rc) return rc;
            d_cand = next;
            per_image = 1;
        }
        if (d_means)   // the mean-scale graph: the curve of round((y - mean) / step)
            rc = basic_gc_rate_curve_ms_dev(d_y, d_scales, d_means, param_stride, sy, nyl, lanes, d_cand, K, per_image,
                                            s->d_table.as<float>(), s->n_scales, s->scale_bound, s->y_tables,
                                            s->d_rate_bits.as<uint64_t>(), st);
        else
            rc = basic_gc_rate_curve_dev(d_y, d_scales, sy, nyl, lanes, d_cand, K, per_image, s->d_table.as<float>(), s->n_scales,
                                         s->scale_bound, s->y_tables, s->d_rate_bits.as<uint64_t>(), st);
        if (!rc)
            rc = basic_rate_select_dev(s->d_rate_bits.as<uint64_t>(), batch, lanes, nyl, d_cand, K, per_image, d_nw_z, d_budget,
                                       d_steps_res, d_choice, d_pred, st);
        if (rc) return rc;
    }
    BASIC_HIP_TRY(hipMemcpyAsync(s->d_steps.p, d_steps_res, sizeof(float) * batch, hipMemcpyDeviceToDevice, st));
    BASIC_HIP_TRY(hipMemcpyAsync(s->h_rate_out.p, s->d_rate_out.p, out_bytes, hipMemcpyDeviceToHost, st));
    return BASIC_OK;
}

// the steps to the device, on the stream whose kernels read them
int upload_qsteps(basic_hp_session *s, hipStream_t st)
{
    const size_t bytes = sizeof(float) * s->qsteps.size();
    if (s->steps_done) BASIC_HIP_TRY(hipEventSynchronize(s->steps_done));   // the previous upload has left h_steps
    else BASIC_HIP_TRY(hipEventCreateWithFlags(&s->steps_done, hipEventDisableTiming));
    int rc = s->h_steps.ensure(bytes);
    if (!rc) rc = s->d_steps.ensure(bytes);
    if (rc) return rc;
    std::memcpy(s->h_steps.p, s->qsteps.data(), bytes);
    BASIC_HIP_TRY(hipMemcpyAsync(s->d_steps.p, s->h_steps.p, bytes, hipMemcpyHostToDevice, st));
    BASIC_HIP_TRY(hipEventRecord(s->steps_done, st));
    return BASIC_OK;
}

// enqueues the encoder of `streams` equal-length streams (n symbols each) into right-aligned slots of `slot` words
int encode_latent(basic_hp_session *s, const basic_rans_tables *t, const int32_t *d_sym, const int32_t *d_idx, int streams,
                  int64_t n, DBuf *seg, DBuf *slots, int32_t *d_nw, int64_t slot, hipStream_t st)
{
    int rc = seg->ensure(sizeof(int64_t) * (streams + 1));
    if (!rc) rc = slots->ensure(sizeof(uint32_t) * static_cast<size_t>(streams) * slot);
    if (rc) return rc;
    hipLaunchKernelGGL(seg_init_kernel, dim3((streams + 256) / 256), dim3(256), 0, st, seg->as<int64_t>(), n, streams,
                       static_cast<int64_t *>(nullptr));
    BASIC_HIP_TRY(hipGetLastError());
    return basic_rans_encode_batch_dev(t, d_sym, d_idx, seg->as<int64_t>(), streams, slots->as<uint32_t>(), slot, d_nw, st);
}

// encode_latent for streams of unequal lengths: d_seg (device, streams + 1 entries) bounds them inside d_sym / d_idx, none longer than
// the slot allows for
int encode_latent_seg(const basic_rans_tables *t, const int32_t *d_sym, const int32_t *d_idx, int streams, const int64_t *d_seg, DBuf *slots,
                      int32_t *d_nw, int64_t slot, hipStream_t st)
{
    const int rc = slots->ensure(sizeof(uint32_t) * static_cast<size_t>(streams) * slot);
    if (rc) return rc;
    return basic_rans_encode_batch_dev(t, d_sym, d_idx, d_seg, streams, slots->as<uint32_t>(), slot, d_nw, st);
}

// the y encoder of a call: equal runs of nyl symbols, or with skip rows their compactions (kept <= nyl: both slot bounds hold)
int encode_y(basic_hp_session *s, int sy, int64_t nyl, int32_t *d_nw_y, int64_t slot_y, hipStream_t st)
{
    if (s->skip_rows == 0)
        return encode_latent(s, s->y_tables, s->y_sym.as<int32_t>(), s->y_idx.as<int32_t>(), sy, nyl, &s->seg_y, &s->slots_y, d_nw_y, slot_y, st);
    return encode_latent_seg(s->y_tables, s->y_symc.as<int32_t>(), s->y_idxc.as<int32_t>(), sy, s->seg_y.as<int64_t>(), &s->slots_y, d_nw_y,
                             slot_y, st);
}

// the buffers of the compaction of sy streams of nyl elements
int ensure_skip(basic_hp_session *s, int sy, int64_t nyl)
{
    int rc = s->skip_scratch.ensure(BASIC_SKIP_SCRATCH_BYTES(sy, nyl));
    if (!rc) rc = s->y_symc.ensure(sizeof(int32_t) * static_cast<size_t>(sy) * nyl);
    if (!rc) rc = s->y_idxc.ensure(sizeof(int32_t) * static_cast<size_t>(sy) * nyl);
    if (!rc) rc = s->seg_y.ensure(sizeof(int64_t) * (sy + 1));
    return rc;
}

// the copy stream and the events that order a session's input buffers between calls
int ensure_copy_stream(basic_hp_session *s)
{
    if (s->copy) return BASIC_OK;
    BASIC_HIP_TRY(hipStreamCreateWithFlags(&s->copy, hipStreamNonBlocking));
    BASIC_HIP_TRY(hipEventCreateWithFlags(&s->x_free, hipEventDisableTiming));
    BASIC_HIP_TRY(hipEventCreateWithFlags(&s->x_ready, hipEventDisableTiming));
    BASIC_HIP_TRY(hipEventCreateWithFlags(&s->u8_free, hipEventDisableTiming));
    BASIC_HIP_TRY(hipEventCreateWithFlags(&s->xhat_free, hipEventDisableTiming));
    return BASIC_OK;
}

// Everything of an encode call behind its input: d_x is float32 [batch][x_channels][h][w] on the device, complete in the order
// of `st`.  x_in_session: d_x is the session's own buffer, whose next writer must wait for this call's analysis transform.
int encode_body(basic_hp_session *s, const float *d_x, bool x_in_session, int batch, int h, int w, uint8_t *out, int64_t out_capacity,
                int64_t *out_len, hipStream_t st)
{
    int rc;
    // ---- inference pass x -> y -> z (latent_graph.py:721-758)
    int yh, yw, zh, zw, ph, pw;
    TokenPhase phase(s, st, &s->enc_phase);   // the analysis transform: ~95 % of the encoder's MFMA work
    if (phase.rc) return phase.rc;
    rc = run_chain(s, s->g_a, d_x, batch, h, w, &s->d_y, nullptr, &yh, &yw, st);
    if (rc) return rc;
    if (x_in_session) {
        BASIC_HIP_TRY(hipEventRecord(s->x_free, st));
        s->x_read_pending = true;
    }
    rc = phase.close();   // the small hyper-path kernels and both rANS stages run beside the next holder's transforms
    if (rc) return rc;
    hipStream_t caller_st = st;
    rc = entropy_stream(s, caller_st, &st);   // from here on `st` is the entropy stream
    if (rc) return rc;
    rc = run_chain(s, s->h_a, s->d_y.as<float>(), batch, yh, yw, &s->d_z, nullptr, &zh, &zw, st);
    if (rc) return rc;
    const int64_t nz = static_cast<int64_t>(s->z_channels) * zh * zw, ny = static_cast<int64_t>(s->y_channels) * yh * yw;
    const int64_t np = s->mean_scale ? 2 * ny : ny;   // prior elements per image: scales, or scales then means
    // lane streams: the y latent of image b is K contiguous runs of ny / K symbols, stream b * K + k (the z path keeps one stream)
    const int K = s->lanes;
    BASIC_REQUIRE(ny % K == 0, "hp_encode_images: stream_lanes does not divide the y latent (channels * h * w) of this call");
    const int sy = batch * K;
    const int64_t nyl = ny / K;
    // ---- node z: EntropyBottleneck symbols + de-quantised latent (compressai_coder.py:203-236), rANS
    rc = s->z_sym.ensure(sizeof(int32_t) * batch * nz);
    if (!rc) rc = s->z_idx.ensure(sizeof(int32_t) * batch * nz);
    if (!rc) rc = s->d_zhat.ensure(sizeof(float) * batch * nz);
    if (!rc) rc = s->nw.ensure(sizeof(int32_t) * (batch + sy));
    if (!rc) rc = s->off.ensure(sizeof(int64_t) * ((batch + 1) + (sy + 1)));
    if (rc) return rc;
    rc = basic_eb_quantize_index_dev(s->d_z.as<float>(), s->d_medians.as<float>(), batch, s->z_channels, zh * zw,
                                     s->z_sym.as<int32_t>(), s->z_idx.as<int32_t>(), s->d_zhat.as<float>(), st);
    if (rc) return rc;
    int64_t slot_z = nz + 2, slot_y = nyl + 2;   // the reference's own buffer size (rans64.cpp:240), per stream
    int32_t *d_nw_z = s->nw.as<int32_t>(), *d_nw_y = s->nw.as<int32_t>() + batch;
    rc = encode_latent(s, s->z_tables, s->z_sym.as<int32_t>(), s->z_idx.as<int32_t>(), batch, nz, &s->seg_z, &s->slots_z, d_nw_z,
                       slot_z, st);
    if (rc) return rc;
    // ---- edge z -> y: h_s(z_hat); node y: GaussianConditional indexes + round (compressai_coder.py:377-385), rANS
    rc = run_chain(s, s->h_s, s->d_zhat.as<float>(), batch, zh, zw, &s->d_prior, nullptr, &ph, &pw, st);
    if (rc) return rc;
    BASIC_REQUIRE(ph >= yh && pw >= yw, "hp_encode_images: the hyper-synthesis output is smaller than the latent");
    const float *d_scales = s->d_prior.as<float>();
    if (ph != yh || pw != yw) {
        rc = s->d_scales.ensure(sizeof(float) * batch * np);
        if (rc) return rc;
        hipLaunchKernelGGL(crop_planes_kernel, dim3(grid_for(batch * np)), dim3(256), 0, st, s->d_prior.as<float>(), ph, pw,
                           s->d_scales.as<float>(), yh, yw, static_cast<int64_t>(batch) * (np / (static_cast<int64_t>(yh) * yw)));
        BASIC_HIP_TRY(hipGetLastError());
        d_scales = s->d_scales.as<float>();
    }
    rc = s->y_sym.ensure(sizeof(int32_t) * batch * ny);
    if (!rc) rc = s->y_idx.ensure(sizeof(int32_t) * batch * ny);
    if (rc) return rc;
    s->rate_res_batch = 0;
    if (s->mean_scale) {
        // the means half of every image's prior follows its scales half: read in place, nothing is copied
        const float *d_means = d_scales + ny, *d_steps = nullptr;
        int n_steps = 0;
        if (!s->rate_budget.empty()) {
            rc = choose_steps(s, s->d_y.as<float>(), d_scales, d_means, np, batch, K, nyl, d_nw_z, st);
            n_steps = batch;
        } else if (!s->qsteps.empty()) {
            rc = upload_qsteps(s, st);
            n_steps = static_cast<int>(s->qsteps.size());
        }
        if (n_steps) d_steps = s->d_steps.as<float>();
        if (!rc)
            rc = basic_gc_quantize_index_ms_dev(s->d_y.as<float>(), d_scales, d_means, batch * ny, ny, np, d_steps, n_steps,
                                                s->d_table.as<float>(), s->n_scales, s->scale_bound, s->y_sym.as<int32_t>(),
                                                s->y_idx.as<int32_t>(), nullptr, st);
    } else if (!s->rate_budget.empty()) {
        rc = choose_steps(s, s->d_y.as<float>(), d_scales, nullptr, 0, batch, K, nyl, d_nw_z, st);
        if (!rc)
            rc = basic_gc_quantize_index_q_dev(s->d_y.as<float>(), d_scales, batch * ny, ny, s->d_steps.as<float>(), batch,
                                               s->d_table.as<float>(), s->n_scales, s->scale_bound, s->y_sym.as<int32_t>(),
                                               s->y_idx.as<int32_t>(), nullptr, st);
    } else if (s->qsteps.empty()) {
        rc = basic_gc_quantize_index_dev(s->d_y.as<float>(), d_scales, batch * ny, s->d_table.as<float>(), s->n_scales, s->scale_bound,
                                         s->y_sym.as<int32_t>(), s->y_idx.as<int32_t>(), nullptr, st);
    } else {
        rc = upload_qsteps(s, st);
        if (!rc)
            rc = basic_gc_quantize_index_q_dev(s->d_y.as<float>(), d_scales, batch * ny, ny, s->d_steps.as<float>(),
                                               static_cast<int>(s->qsteps.size()), s->d_table.as<float>(), s->n_scales, s->scale_bound,
                                               s->y_sym.as<int32_t>(), s->y_idx.as<int32_t>(), nullptr, st);
    }
    if (rc) return rc;
    if (s->skip_rows) {   // the streams shrink to the elements whose row is at least skip_rows, each run on its own
        rc = ensure_skip(s, sy, nyl);
        if (!rc)
            rc = basic_skip_compact_dev(s->y_sym.as<int32_t>(), s->y_idx.as<int32_t>(), sy, nyl, s->skip_rows, s->skip_scratch.p,
                                        s->y_symc.as<int32_t>(), s->y_idxc.as<int32_t>(), s->seg_y.as<int64_t>(), st);
        if (rc) return rc;
    }
    rc = encode_y(s, sy, nyl, d_nw_y, slot_y, st);
    if (rc) return rc;
    // ---- stream lengths to the host; offsets and compaction on the device meanwhile
    rc = s->h_nw.ensure(sizeof(int32_t) * (batch + sy));
    if (rc) return rc;
    int32_t *h_nw = s->h_nw.as<int32_t>();
    for (int attempt = 0;; ++attempt) {
        int64_t *d_off_z = s->off.as<int64_t>(), *d_off_y = s->off.as<int64_t>() + (batch + 1);
        hipLaunchKernelGGL(offsets_kernel, dim3(1), dim3(64), 0, st, d_nw_z, batch, d_off_z);
        hipLaunchKernelGGL(offsets_kernel, dim3(1), dim3(64), 0, st, d_nw_y, sy, d_off_y);
        BASIC_HIP_TRY(hipGetLastError());
        // both latents' streams share one packed buffer: z first, then y (each at its own base)
        rc = s->packed.ensure(sizeof(uint32_t) * (static_cast<size_t>(batch) * slot_z + static_cast<size_t>(sy) * slot_y));
        if (rc) return rc;
        uint32_t *d_pz = s->packed.as<uint32_t>(), *d_py = d_pz + static_cast<size_t>(batch) * slot_z;
        rc = basic_rans_compact_streams_dev(s->slots_z.as<uint32_t>(), slot_z, d_nw_z, d_off_z, batch, d_pz, st);
        if (!rc) rc = basic_rans_compact_streams_dev(s->slots_y.as<uint32_t>(), slot_y, d_nw_y, d_off_y, sy, d_py, st);
        if (rc) return rc;
        BASIC_HIP_TRY(hipMemcpyAsync(h_nw, s->nw.p, sizeof(int32_t) * (batch + sy), hipMemcpyDeviceToHost, st));
        BASIC_HIP_TRY(hipStreamSynchronize(st));
        bool over_z = false, over_y = false;
        for (int i = 0; i < batch; ++i) over_z |= h_nw[i] < 0;
        for (int i = 0; i < sy; ++i) over_y |= h_nw[batch + i] < 0;
        if (!over_z && !over_y) break;
        BASIC_REQUIRE(attempt == 0, "hp_encode_images: rANS slot overflow with the guaranteed slot size");
        // bypass-heavy data overflowed the reference's bound (undefined behaviour there): redo with the guaranteed one
        if (over_z) {
            slot_z = 3 * nz + 4;
            rc = encode_latent(s, s->z_tables, s->z_sym.as<int32_t>(), s->z_idx.as<int32_t>(), batch, nz, &s->seg_z, &s->slots_z, d_nw_z,
                               slot_z, st);
            if (rc) return rc;
        }
        if (over_y) {
            slot_y = 3 * nyl + 4;   // guaranteed per lane stream
            rc = encode_y(s, sy, nyl, d_nw_y, slot_y, st);
            if (rc) return rc;
        }
    }
    s->off_z.assign(batch + 1, 0);
    s->off_y.assign(sy + 1, 0);
    for (int i = 0; i < batch; ++i) s->off_z[i + 1] = s->off_z[i] + h_nw[i];
    for (int i = 0; i < sy; ++i) s->off_y[i + 1] = s->off_y[i] + h_nw[batch + i];
    const int64_t wz = s->off_z[batch], wy = s->off_y[sy];
    rc = s->h_words.ensure(sizeof(uint32_t) * static_cast<size_t>(wz + wy));
    if (rc) return rc;
    uint32_t *h_wz = s->h_words.as<uint32_t>(), *h_wy = h_wz + wz;
    const uint32_t *d_pz = s->packed.as<uint32_t>(), *d_py = d_pz + static_cast<size_t>(batch) * slot_z;
    if (wz) BASIC_HIP_TRY(hipMemcpyAsync(h_wz, d_pz, sizeof(uint32_t) * wz, hipMemcpyDeviceToHost, st));
    if (wy) BASIC_HIP_TRY(hipMemcpyAsync(h_wy, d_py, sizeof(uint32_t) * wy, hipMemcpyDeviceToHost, st));
    BASIC_HIP_TRY(hipStreamSynchronize(st));
    rc = rejoin(s, caller_st, st);
    if (rc) return rc;
    if (!s->rate_budget.empty()) s->rate_res_batch = batch;
    s->res_batch = batch; s->res_lanes = K; s->res_zh = zh; s->res_zw = zw; s->res_yh = yh; s->res_yw = yw;
    *out_len = 4 + (12 + 4ll * batch + 4 * wz) + (12 + 4ll * sy + 4 * wy);
    if (!out) return BASIC_OK;   // the caller fetches the bytes with basic_hp_encode_result() once it knows their size
    return basic_hp_encode_result(s, out, out_capacity, out_len);
}

}  // namespace

extern "C" int basic_hp_encode_images(basic_hp_session *s, const float *x, int x_on_host, int batch, int h, int w, uint8_t *out,
                                      int64_t out_capacity, int64_t *out_len, void *hip_stream)
{
    BASIC_REQUIRE(s && x && out_len && batch >= 1 && h >= 1 && w >= 1, "hp_encode_images: bad argument");
    BASIC_REQUIRE(qsteps_fit(s, batch), "hp_encode_images: the session's quantiser steps are neither one nor one per image of this batch");
    BASIC_REQUIRE(budgets_fit(s, batch), "hp_encode_images: the session's byte budgets are neither one nor one per image of this batch");
    s->res_batch = 0;
    hipStream_t st = as_stream(hip_stream);
    WavesGuard guard(s->rans_waves, s->use_token);
    int rc;
    const float *d_x = x;
    if (x_on_host) {   // general_codec.py:46-47: the upload belongs to compress()
        const size_t bytes = sizeof(float) * static_cast<size_t>(batch) * s->x_channels * h * w;
        rc = s->d_x.ensure(bytes);
        if (!rc) rc = ensure_copy_stream(s);
        if (rc) return rc;
        if (s->x_read_pending) BASIC_HIP_TRY(hipStreamWaitEvent(s->copy, s->x_free, 0));
        BASIC_HIP_TRY(hipMemcpyAsync(s->d_x.p, x, bytes, hipMemcpyHostToDevice, s->copy));
        BASIC_HIP_TRY(hipEventRecord(s->x_ready, s->copy));
        BASIC_HIP_TRY(hipStreamWaitEvent(st, s->x_ready, 0));
        d_x = s->d_x.as<float>();
    }
    return encode_body(s, d_x, x_on_host != 0, batch, h, w, out, out_capacity, out_len, st);
}

// The uint8 batch reaches d_x through a conversion on the caller's stream.  Orders kept between calls (whose streams may differ):
// the upload into u8_in waits for the previous conversion out of it (u8_free); the conversion waits for the upload (x_ready) and,
// as the float upload does, for the previous call's analysis transform, the last reader of d_x (x_free).
extern "C" int basic_hp_encode_images_u8(basic_hp_session *s, const uint8_t *x, int x_on_host, int layout, int batch, int h, int w,
                                         uint8_t *out, int64_t out_capacity, int64_t *out_len, void *hip_stream)
{
    BASIC_REQUIRE(s && x && out_len && batch >= 1 && h >= 1 && w >= 1, "hp_encode_images_u8: bad argument");
    BASIC_REQUIRE(layout == BASIC_IMAGE_CHW || layout == BASIC_IMAGE_HWC, "hp_encode_images_u8: layout is BASIC_IMAGE_CHW or BASIC_IMAGE_HWC");
    BASIC_REQUIRE(qsteps_fit(s, batch), "hp_encode_images_u8: the session's quantiser steps are neither one nor one per image of this batch");
    BASIC_REQUIRE(budgets_fit(s, batch), "hp_encode_images_u8: the session's byte budgets are neither one nor one per image of this batch");
    s->res_batch = 0;
    hipStream_t st = as_stream(hip_stream);
    WavesGuard guard(s->rans_waves, s->use_token);
    const size_t samples = static_cast<size_t>(batch) * s->x_channels * h * w;
    int rc = s->d_x.ensure(sizeof(float) * samples);
    if (!rc) rc = ensure_copy_stream(s);
    if (rc) return rc;
    const uint8_t *d_u8 = x;
    if (x_on_host) {
        rc = s->u8_in.ensure(samples);
        if (rc) return rc;
        if (s->u8_read_pending) BASIC_HIP_TRY(hipStreamWaitEvent(s->copy, s->u8_free, 0));
        BASIC_HIP_TRY(hipMemcpyAsync(s->u8_in.p, x, samples, hipMemcpyHostToDevice, s->copy));
        BASIC_HIP_TRY(hipEventRecord(s->x_ready, s->copy));
        BASIC_HIP_TRY(hipStreamWaitEvent(st, s->x_ready, 0));
        d_u8 = s->u8_in.as<uint8_t>();
    }
    if (s->x_read_pending) BASIC_HIP_TRY(hipStreamWaitEvent(st, s->x_free, 0));
    rc = basic_image_u8_to_f32_dev(d_u8, layout, batch, s->x_channels, h, w, s->d_x.as<float>(), st);
    if (rc) return rc;
    if (x_on_host) {
        BASIC_HIP_TRY(hipEventRecord(s->u8_free, st));
        s->u8_read_pending = true;
    }
    return encode_body(s, s->d_x.as<float>(), true, batch, h, w, out, out_capacity, out_len, st);
}

// framing: merge_bytes([z body, y body], num_segments=2) with write_body bodies (bytes_ops.py:19-33)
extern "C" int basic_hp_encode_result(basic_hp_session *s, uint8_t *out, int64_t out_capacity, int64_t *out_len)
{
    BASIC_REQUIRE(s && out && s->res_batch >= 1, "hp_encode_result: no encoded batch is held by this session");
    const int batch = s->res_batch, sy = batch * s->res_lanes;   // y body: the tabled form for batch * lanes streams
    const int64_t wz = s->off_z[batch], wy = s->off_y[sy];
    const uint32_t *h_wz = s->h_words.as<uint32_t>(), *h_wy = h_wz + wz;
    const int64_t len_z = 12 + 4ll * batch + 4 * wz, len_y = 12 + 4ll * sy + 4 * wy;
    if (out_len) *out_len = 4 + len_z + len_y;
    if (4 + len_z + len_y > out_capacity) { set_error("hp_encode_result: output buffer too small"); return BASIC_ERR_OVERFLOW; }
    BASIC_REQUIRE(len_z <= 0xFFFFFFFFll, "hp_encode_result: z body exceeds the 32-bit length prefix");
    const uint32_t lz32 = static_cast<uint32_t>(len_z);
    std::memcpy(out, &lz32, 4);   // native-endian struct "I"
    int64_t written = 0;
    int rc = basic_frame_streams(h_wz, s->off_z.data(), batch, static_cast<uint32_t>(s->res_zh), static_cast<uint32_t>(s->res_zw), out + 4,
                                 len_z, &written);
    if (rc) return rc;
    return basic_frame_streams(h_wy, s->off_y.data(), sy, static_cast<uint32_t>(s->res_yh), static_cast<uint32_t>(s->res_yw),
                               out + 4 + len_z, len_y, &written);
}

namespace {

struct Body {
    const uint8_t *p = nullptr;
    int64_t len = 0;
    uint32_t h = 0, w = 0;
    int n = 0;
};

int split_bodies(const uint8_t *data, int64_t len, int lanes, Body *z, Body *y)
{
    BASIC_REQUIRE(data && len >= 4 + 12 + 12, "hp_decode_images: truncated stream");
    uint32_t lz = 0;
    std::memcpy(&lz, data, 4);
    BASIC_REQUIRE(4ll + lz + 12 <= len && lz >= 12, "hp_decode_images: bad z-body length");
    z->p = data + 4; z->len = lz;
    y->p = data + 4 + lz; y->len = len - 4 - lz;
    int rc = basic_unframe_streams(z->p, z->len, &z->h, &z->w, &z->n, nullptr, 0, nullptr);
    if (!rc) rc = basic_unframe_streams(y->p, y->len, &y->h, &y->w, &y->n, nullptr, 0, nullptr);
    if (rc) return rc;
    BASIC_REQUIRE(z->n >= 1 && static_cast<int64_t>(y->n) == static_cast<int64_t>(z->n) * lanes,
                  "hp_decode_images: the y body does not hold stream_lanes streams for every stream of the z body");
    return BASIC_OK;
}

}  // namespace

extern "C" int basic_hp_decoded_shape(const basic_hp_session *s, const uint8_t *data, int64_t len, int *batch, int *channels, int *h,
                                      int *w)
{
    BASIC_REQUIRE(s, "hp_decoded_shape: null session");
    Body z, y;
    int rc = split_bodies(data, len, s->lanes, &z, &y);
    if (rc) return rc;
    int oh, ow;
    rc = chain_out_hw(s->g_s, static_cast<int>(y.h), static_cast<int>(y.w), &oh, &ow);
    if (rc) return rc;
    if (batch) *batch = z.n;
    if (channels) *channels = s->out_channels;
    if (h) *h = oh;
    if (w) *w = ow;
    return BASIC_OK;
}

namespace {

// a decode call: the reconstruction goes to d_xhat (float32 on the device), enqueued on `st`
int decode_body(basic_hp_session *s, const uint8_t *data, int64_t len, float *d_xhat, int64_t xhat_capacity_floats, hipStream_t st)
{
    WavesGuard guard(s->rans_waves, s->use_token);
    Body z, y;
    int rc = split_bodies(data, len, s->lanes, &z, &y);
    if (rc) return rc;
    hipStream_t caller_st = st;
    rc = entropy_stream(s, caller_st, &st);   // everything before g_s goes to the entropy stream
    if (rc) return rc;
    const int batch = z.n, sy = y.n, K = s->lanes, zh = z.h, zw = z.w, yh = y.h, yw = y.w;
    BASIC_REQUIRE(qsteps_fit(s, batch), "hp_decode_images: the session's quantiser steps are neither one nor one per image of this stream");
    int oh, ow;
    rc = chain_out_hw(s->g_s, yh, yw, &oh, &ow);
    if (rc) return rc;
    BASIC_REQUIRE(static_cast<int64_t>(batch) * s->out_channels * oh * ow <= xhat_capacity_floats, "hp_decode_images: output buffer too small");
    const int64_t nz = static_cast<int64_t>(s->z_channels) * zh * zw, ny = static_cast<int64_t>(s->y_channels) * yh * yw;
    const int64_t np = s->mean_scale ? 2 * ny : ny;   // prior elements per image: scales, or scales then means
    BASIC_REQUIRE(ny % K == 0, "hp_decode_images: stream_lanes does not divide the y latent (channels * h * w) of this stream");
    const int64_t nyl = ny / K;   // y: stream b * K + k continues image b at symbol k * nyl -- contiguous runs of [B][ny]
    // ---- unframe both bodies into ONE pinned staging area [z words | y words | z offsets | y offsets] and upload it
    const int64_t wz = (z.len - 12 - 4ll * batch) / 4, wy = (y.len - 12 - 4ll * sy) / 4;
    BASIC_REQUIRE(wz >= 0 && wy >= 0, "hp_decode_images: truncated body");
    const size_t words_bytes = sizeof(uint32_t) * static_cast<size_t>(wz + wy + 2);
    const size_t off_pad = (words_bytes + 7) & ~static_cast<size_t>(7);
    const size_t total = off_pad + sizeof(int64_t) * ((batch + 1) + (sy + 1));
    if (s->in_done) BASIC_HIP_TRY(hipEventSynchronize(s->in_done));   // the previous call's upload out of h_in has finished
    else BASIC_HIP_TRY(hipEventCreateWithFlags(&s->in_done, hipEventDisableTiming));
    rc = s->h_in.ensure(total);
    if (!rc) rc = s->words.ensure(total);
    if (rc) return rc;
    uint8_t *hb = s->h_in.as<uint8_t>();
    uint32_t *h_wz = reinterpret_cast<uint32_t *>(hb), *h_wy = h_wz + wz;
    int64_t *h_oz = reinterpret_cast<int64_t *>(hb + off_pad), *h_oy = h_oz + (batch + 1);
    uint32_t hh, ww;
    int nn;
    rc = basic_unframe_streams(z.p, z.len, &hh, &ww, &nn, h_oz, batch, h_wz);
    if (!rc) rc = basic_unframe_streams(y.p, y.len, &hh, &ww, &nn, h_oy, sy, h_wy);
    if (rc) return rc;
    BASIC_HIP_TRY(hipMemcpyAsync(s->words.p, hb, total, hipMemcpyHostToDevice, st));
    BASIC_HIP_TRY(hipEventRecord(s->in_done, st));
    const uint8_t *db = s->words.as<uint8_t>();
    const uint32_t *d_wz = reinterpret_cast<const uint32_t *>(db), *d_wy = d_wz + wz;
    const int64_t *d_oz = reinterpret_cast<const int64_t *>(db + off_pad), *d_oy = d_oz + (batch + 1);
    // ---- node z: indexes = channel, rANS decode, de-quantise (compressai_coder.py:238-245)
    rc = s->z_sym.ensure(sizeof(int32_t) * batch * nz);
    if (!rc) rc = s->z_idx.ensure(sizeof(int32_t) * batch * nz);
    if (!rc) rc = s->d_zhat.ensure(sizeof(float) * batch * nz);
    if (!rc) rc = s->seg_z.ensure(sizeof(int64_t) * (batch + 1));
    if (!rc) rc = s->seg_y.ensure(sizeof(int64_t) * (sy + 1));
    if (!rc) rc = s->state.ensure(sizeof(uint64_t) * (batch + sy));
    if (!rc) rc = s->pos.ensure(sizeof(int64_t) * (batch + sy));
    if (rc) return rc;
    hipLaunchKernelGGL(channel_index_kernel, dim3(grid_for(batch * nz)), dim3(256), 0, st, s->z_idx.as<int32_t>(), s->z_channels, zh * zw,
                       batch * nz);
    hipLaunchKernelGGL(seg_init_kernel, dim3((batch + 256) / 256), dim3(256), 0, st, s->seg_z.as<int64_t>(), nz, batch, s->pos.as<int64_t>());
    hipLaunchKernelGGL(seg_init_kernel, dim3((sy + 256) / 256), dim3(256), 0, st, s->seg_y.as<int64_t>(), nyl, sy,
                       s->pos.as<int64_t>() + batch);
    BASIC_HIP_TRY(hipGetLastError());
    rc = basic_rans_decode_batch_dev(s->z_tables, d_wz, d_oz, s->z_idx.as<int32_t>(), s->seg_z.as<int64_t>(), batch, s->z_sym.as<int32_t>(),
                                     s->state.as<uint64_t>(), s->pos.as<int64_t>(), st);
    if (rc) return rc;
    rc = basic_eb_dequantize_dev(s->z_sym.as<int32_t>(), s->d_medians.as<float>(), batch, s->z_channels, zh * zw, s->d_zhat.as<float>(), st);
    if (rc) return rc;
    // ---- edge z -> y, node y (compressai_coder.py:387-393)
    int ph, pw;
    rc = run_chain(s, s->h_s, s->d_zhat.as<float>(), batch, zh, zw, &s->d_prior, nullptr, &ph, &pw, st);
    if (rc) return rc;
    BASIC_REQUIRE(ph >= yh && pw >= yw, "hp_decode_images: the hyper-synthesis output is smaller than the latent");
    const float *d_scales = s->d_prior.as<float>();
    if (ph != yh || pw != yw) {
        rc = s->d_scales.ensure(sizeof(float) * batch * np);
        if (rc) return rc;
        hipLaunchKernelGGL(crop_planes_kernel, dim3(grid_for(batch * np)), dim3(256), 0, st, s->d_prior.as<float>(), ph, pw,
                           s->d_scales.as<float>(), yh, yw, static_cast<int64_t>(batch) * (np / (static_cast<int64_t>(yh) * yw)));
        BASIC_HIP_TRY(hipGetLastError());
        d_scales = s->d_scales.as<float>();
    }
    rc = s->y_sym.ensure(sizeof(int32_t) * batch * ny);
    if (!rc) rc = s->y_idx.ensure(sizeof(int32_t) * batch * ny);
    if (!rc) rc = s->d_y.ensure(sizeof(float) * batch * ny);
    if (rc) return rc;
    // indexes only: the symbol output of this launch is scratch (the module path does the same, compressai_coder.py:387-393)
    const int n_steps = static_cast<int>(s->qsteps.size());
    if (s->mean_scale) {
        if (n_steps) rc = upload_qsteps(s, st);
        if (!rc)
            rc = basic_gc_quantize_index_ms_dev(nullptr, d_scales, nullptr, batch * ny, ny, np, n_steps ? s->d_steps.as<float>() : nullptr,
                                                n_steps, s->d_table.as<float>(), s->n_scales, s->scale_bound, nullptr,
                                                s->y_idx.as<int32_t>(), nullptr, st);
    } else if (!n_steps) {
        rc = basic_gc_quantize_index_dev(d_scales, d_scales, batch * ny, s->d_table.as<float>(), s->n_scales, s->scale_bound,
                                         s->y_sym.as<int32_t>(), s->y_idx.as<int32_t>(), nullptr, st);
    } else {
        rc = upload_qsteps(s, st);
        if (!rc)
            rc = basic_gc_quantize_index_q_dev(d_scales, d_scales, batch * ny, ny, s->d_steps.as<float>(), n_steps, s->d_table.as<float>(),
                                               s->n_scales, s->scale_bound, s->y_sym.as<int32_t>(), s->y_idx.as<int32_t>(), nullptr, st);
    }
    if (rc) return rc;
    if (s->skip_rows) {
        // the streams hold the elements whose row is at least skip_rows: compact the indexes (seg_y becomes the streams' bounds),
        // decode into the compact array, put the symbols back where they belong with 0 in between
        rc = ensure_skip(s, sy, nyl);
        if (!rc)
            rc = basic_skip_compact_dev(nullptr, s->y_idx.as<int32_t>(), sy, nyl, s->skip_rows, s->skip_scratch.p, nullptr,
                                        s->y_idxc.as<int32_t>(), s->seg_y.as<int64_t>(), st);
        if (!rc)
            rc = basic_rans_decode_batch_dev(s->y_tables, d_wy, d_oy, s->y_idxc.as<int32_t>(), s->seg_y.as<int64_t>(), sy,
                                             s->y_symc.as<int32_t>(), s->state.as<uint64_t>() + batch, s->pos.as<int64_t>() + batch, st);
        if (!rc)
            rc = basic_skip_expand_dev(s->y_symc.as<int32_t>(), s->y_idx.as<int32_t>(), sy, nyl, s->skip_rows, s->skip_scratch.p,
                                       s->y_sym.as<int32_t>(), st);
    } else {
        rc = basic_rans_decode_batch_dev(s->y_tables, d_wy, d_oy, s->y_idx.as<int32_t>(), s->seg_y.as<int64_t>(), sy, s->y_sym.as<int32_t>(),
                                         s->state.as<uint64_t>() + batch, s->pos.as<int64_t>() + batch, st);
    }
    if (rc) return rc;
    if (s->mean_scale)
        rc = basic_gc_dequantize_ms_dev(s->y_sym.as<int32_t>(), d_scales + ny, batch * ny, ny, np, n_steps ? s->d_steps.as<float>() : nullptr,
                                        n_steps, s->d_y.as<float>(), st);
    else if (!n_steps) rc = basic_i32_to_f32_dev(s->y_sym.as<int32_t>(), batch * ny, s->d_y.as<float>(), st);
    else rc = basic_gc_dequantize_q_dev(s->y_sym.as<int32_t>(), batch * ny, ny, s->d_steps.as<float>(), n_steps, s->d_y.as<float>(), st);
    if (rc) return rc;
    // ---- edge y -> x: g_s straight into the caller's buffer
    rc = rejoin(s, caller_st, st);
    if (rc) return rc;
    st = caller_st;
    TokenPhase phase(s, st, &s->dec_phase);
    if (phase.rc) return phase.rc;
    rc = run_chain(s, s->g_s, s->d_y.as<float>(), batch, yh, yw, nullptr, d_xhat, nullptr, nullptr, st);
    const int rc2 = phase.close();
    return rc ? rc : rc2;
}

}  // namespace

extern "C" int basic_hp_decode_images(basic_hp_session *s, const uint8_t *data, int64_t len, float *d_xhat,
                                      int64_t xhat_capacity_floats, void *hip_stream)
{
    BASIC_REQUIRE(s && d_xhat, "hp_decode_images: bad argument");
    return decode_body(s, data, len, d_xhat, xhat_capacity_floats, as_stream(hip_stream));
}

extern "C" int basic_hp_decode_images_u8(basic_hp_session *s, const uint8_t *data, int64_t len, int layout, uint8_t *xhat,
                                         int xhat_on_host, int64_t xhat_capacity_bytes, void *hip_stream)
{
    BASIC_REQUIRE(s && xhat, "hp_decode_images_u8: bad argument");
    BASIC_REQUIRE(layout == BASIC_IMAGE_CHW || layout == BASIC_IMAGE_HWC, "hp_decode_images_u8: layout is BASIC_IMAGE_CHW or BASIC_IMAGE_HWC");
    int batch = 0, channels = 0, h = 0, w = 0;
    int rc = basic_hp_decoded_shape(s, data, len, &batch, &channels, &h, &w);
    if (rc) return rc;
    BASIC_REQUIRE(batch >= 1 && channels >= 1 && h >= 1 && w >= 1, "hp_decode_images_u8: the stream states an empty picture");
    const int64_t samples = static_cast<int64_t>(batch) * channels * h * w;
    BASIC_REQUIRE(samples <= xhat_capacity_bytes, "hp_decode_images_u8: output buffer too small");
    hipStream_t st = as_stream(hip_stream);
    rc = s->d_xhat.ensure(sizeof(float) * static_cast<size_t>(samples));
    if (!rc && xhat_on_host) rc = s->u8_out.ensure(static_cast<size_t>(samples));
    if (!rc) rc = ensure_copy_stream(s);
    if (rc) return rc;
    // the previous call's conversion out of d_xhat may have run on another stream
    if (s->xhat_read_pending) BASIC_HIP_TRY(hipStreamWaitEvent(st, s->xhat_free, 0));
    rc = decode_body(s, data, len, s->d_xhat.as<float>(), samples, st);
    if (rc) return rc;
    uint8_t *d_u8 = xhat_on_host ? s->u8_out.as<uint8_t>() : xhat;
    rc = basic_image_f32_to_u8_dev(s->d_xhat.as<float>(), batch, channels, h, w, layout, d_u8, st);
    if (rc) return rc;
    BASIC_HIP_TRY(hipEventRecord(s->xhat_free, st));
    s->xhat_read_pending = true;
    if (xhat_on_host) {   // u8_out is read by this copy alone, and the copy is over when the call returns
        BASIC_HIP_TRY(hipMemcpyAsync(xhat, d_u8, static_cast<size_t>(samples), hipMemcpyDeviceToHost, st));
        BASIC_HIP_TRY(hipStreamSynchronize(st));
    }
    return BASIC_OK;
}
