// Window groups: the greedy single-token steps of up to 8 batch-Whisper windows (different sessions of one model) as ONE
// launch chain - one pass over the decoder weights per token for all of them.
//
// `transcribe()` drives each 30 s window from Python, one wlk_decode + one wlk_pick_greedy per token; eight concurrent
// LocalAgreement sessions therefore stream the decoder weights eight times per token.  A wlk_group owns a stream and the
// activation workspace of an R <= 8 row step; wlk_group_step_pick takes the next token of n sessions, runs the decoder
// layers over the n rows with the per-row kernels the batch engine uses (every row reads and extends ITS session's caches
// through a StepRow table), projects onto the vocabulary, applies each row's logit rules and greedy pick
// (select.hip: rules_pick_rows_kernel) and reads 8 n bytes back.  The loop over tokens stays on the host: one library call
// per token for all rows, no thread, no wait on host-coherent flags and no graph inside the library (the chain as one graph
// replay per row count was measured and did not pay: DESIGN 26).
//
// The layer chain restates wlk_engine::enqueue_decoder (engine.hip) with one difference: the cross-attention's query
// projection is the multi-row GEMV for EVERY row count, also for one row (the engine folds it into the attention kernel
// there).  A row therefore goes through the same kernels whether it steps alone or beside seven others.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <mutex>

#include "common.h"
#include "internal.h"

using namespace wlk;

namespace {
constexpr int kGroupMaxRows = 8;
// what one step uploads, in one copy: the row table the layer kernels index and the rule table of the pick
struct GroupBlock {
    StepRow rows[kGroupMaxRows];
    PickRowEntry pick[kGroupMaxRows];
};
}  // namespace

struct wlk_group {
    wlk_model* m = nullptr;
    int max_rows = 1;
    hipStream_t stream = nullptr;
    float *x = nullptr, *qkv = nullptr, *att = nullptr, *q = nullptr, *mlp = nullptr, *logits = nullptr, *xsplit = nullptr;
    GroupBlock* blk_dev = nullptr;
    int* pick_dev = nullptr;             // [R][token | log-probability]
    char* pinned = nullptr;              // [GroupBlock | R x 8 bytes of results]
    hipEvent_t joined[kGroupMaxRows] = {};
    int last_rows = 0;                   // rows of the last completed step (wlk_group_export_logits)
    uint64_t n_steps = 0, n_rows = 0;
    std::mutex mu;                       // one step at a time

    ~wlk_group() {
        (void)hipSetDevice(m->device);
        if (stream) (void)hipStreamSynchronize(stream);
        float* fl[] = {x, qkv, att, q, mlp, logits, xsplit};
        for (float* p : fl)
            if (p) (void)hipFree(p);
        if (blk_dev) (void)hipFree(blk_dev);
        if (pick_dev) (void)hipFree(pick_dev);
        if (pinned) (void)hipHostFree(pinned);
        for (hipEvent_t e : joined)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }

    void enqueue_step(int R);
};

// embed .. logits of R rows + every row's pick: wlk_engine::enqueue_decoder's operators in its order (see the file comment)
void wlk_group::enqueue_step(int R) {
    const wlk_dims& D = m->D;
    const int d = D.n_text_state, T = D.n_audio_ctx, H = D.n_text_head, V = D.n_vocab, ctx_len = D.n_text_ctx;
    const LaunchCtx c{stream, nullptr};
    const float scale = std::pow((float)kHeadDim, -0.25f);
    const StepRow* rows_dev = blk_dev->rows;
    launch_embed_rows(c, rows_dev, m->w_tok_emb, m->w_dec_pos, x, R, d);
    float* sc = xsplit;
    float* pm = sc + (size_t)8 * H * T;
    float* pl = pm + (size_t)8 * H * 8;
    float* po = pl + (size_t)8 * H * 8;
    for (int i = 0; i < D.n_text_layer; ++i) {
        const LayerW& L = m->dec_layers[i];
        const long layer_off = (long)i * ctx_len * d;       // beam 1: [L][ctx][d]
        GemmArgs g;
        g.A = x; g.lda = d; g.W = L.qkvw; g.bias = L.qkvb; g.C = qkv; g.ldc = 3 * d; g.M = R; g.N = 3 * d; g.K = d;
        g.flags = kGemmScaleCols; g.scale = scale; g.scale_cols = 2 * d;
        g.ln_gamma = L.ln1w; g.ln_beta = L.ln1b;
        g.kv_rows = rows_dev; g.kv_layer_off = layer_off; g.kv_d = d; g.kv_ctx = ctx_len;
        launch_gemv(c, g, "dec_ln1_qkv_kv");
        launch_decoder_self_attention_rows(c, qkv, rows_dev, layer_off, att, R, d, H, ctx_len);
        GemmArgs o;
        o.A = att; o.lda = d; o.W = L.outw; o.bias = L.outb; o.C = x; o.ldc = d; o.M = R; o.N = d; o.K = d;
        o.flags = kGemmResidual; o.R = x; o.ldr = d;
        launch_gemv(c, o, "dec_out");
        GemmArgs qq;
        qq.A = x; qq.lda = d; qq.W = L.xqw; qq.bias = L.xqb; qq.C = q; qq.ldc = d; qq.M = R; qq.N = d; qq.K = d;
        qq.flags = kGemmScaleCols; qq.scale = scale; qq.scale_cols = d; qq.ln_gamma = L.lnxw; qq.ln_beta = L.lnxb;
        launch_gemv(c, qq, "dec_lnx_xq");
        CrossAttnArgs ca{};
        ca.q = q; ca.k = nullptr; ca.v = nullptr; ca.ldkv = (long)D.n_text_layer * 2 * d; ca.out = att;
        ca.rows = R; ca.d = d; ca.n_head = H; ca.T = T;
        ca.head_rank = m->n_align > 0 ? m->head_rank + (size_t)i * H : nullptr;
        ca.ring = nullptr; ca.ring_row = nullptr; ca.beam_of_row = nullptr;
        ca.ring_rows = ctx_len + kAlignWindow; ca.n_beam = 1; ca.qk_debug = nullptr;
        ca.step_rows = rows_dev; ca.kv_off = (long)i * 2 * d;
        launch_decoder_cross_attention_split(c, ca, sc, pm, pl, po, true);
        GemmArgs xo;
        xo.A = att; xo.lda = d; xo.W = L.xoutw; xo.bias = L.xoutb; xo.C = x; xo.ldc = d; xo.M = R; xo.N = d; xo.K = d;
        xo.flags = kGemmResidual; xo.R = x; xo.ldr = d;
        launch_gemv(c, xo, "dec_xout");
        GemmArgs f1;
        f1.A = x; f1.lda = d; f1.W = L.fc1w; f1.bias = L.fc1b; f1.C = mlp; f1.ldc = 4 * d; f1.M = R; f1.N = 4 * d; f1.K = d;
        f1.flags = kGemmGelu; f1.ln_gamma = L.ln2w; f1.ln_beta = L.ln2b;
        launch_gemv(c, f1, "dec_ln2_fc1");
        GemmArgs f2;
        f2.A = mlp; f2.lda = 4 * d; f2.W = L.fc2w; f2.bias = L.fc2b; f2.C = x; f2.ldc = d; f2.M = R; f2.N = d; f2.K = 4 * d;
        f2.flags = kGemmResidual; f2.R = x; f2.ldr = d;
        launch_gemv(c, f2, "dec_fc2");
    }
    GemmArgs lg;
    lg.A = x; lg.lda = d; lg.W = m->w_tok_emb; lg.C = logits; lg.ldc = V; lg.M = R; lg.N = V; lg.K = d;
    lg.ln_gamma = m->w_ln_w; lg.ln_beta = m->w_ln_b;
    launch_gemv(c, lg, "dec_lnf_logits");
    launch_rules_pick_rows(c, logits, V, R, blk_dev->pick, pick_dev);
}

static bool pick_params_ok(const wlk_pick_params& p, int V) {
    return p.timestamp_begin >= 0 && p.timestamp_begin <= V && p.eot >= 0 && p.eot < V && p.ts_mode >= 0 && p.ts_mode <= 2;
}
static PickRules pick_rules_of(const wlk_pick_params& p) {
    return PickRules{p.first_step, p.without_timestamps, p.timestamp_begin, p.eot, p.no_timestamps, p.ts_mode, p.ts_bound,
                     p.max_initial};
}

extern "C" {

int wlk_group_create(wlk_model* m, int max_rows, wlk_group** out) {
    if (!m || !out) return fail(WLK_ERR_ARG, "NULL argument");
    if (!m->finalized) return fail(WLK_ERR_STATE, "model not finalized");
    if (max_rows < 1 || max_rows > kGroupMaxRows) return fail(WLK_ERR_ARG, "window group: 1..8 rows");
    if (!gemv_applicable(max_rows, 4 * m->D.n_text_state))
        return fail(WLK_ERR_ARG, "window group: the model is too wide for that many stacked single-token rows");
    return guarded([&]() {
        WLK_HIP(hipSetDevice(m->device));
        auto g = std::make_unique<wlk_group>();
        g->m = m;
        g->max_rows = max_rows;
        WLK_HIP(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
        const wlk_dims& D = m->D;
        const size_t R = kGroupMaxRows, d = D.n_text_state, T = D.n_audio_ctx, V = D.n_vocab;
        g->x = dev_alloc<float>(R * d);
        g->qkv = dev_alloc<float>(R * 3 * d);
        g->att = dev_alloc<float>(R * d);
        g->q = dev_alloc<float>(R * d);
        g->mlp = dev_alloc<float>(R * 4 * d);
        g->logits = dev_alloc<float>(R * V);
        g->xsplit = dev_alloc<float>(cross_split_scratch_floats(8, D.n_text_head, (int)T));
        g->blk_dev = reinterpret_cast<GroupBlock*>(dev_alloc<char>(sizeof(GroupBlock)));
        g->pick_dev = dev_alloc<int>(2 * R);
        WLK_HIP(hipHostMalloc(reinterpret_cast<void**>(&g->pinned), sizeof(GroupBlock) + 8 * R, hipHostMallocDefault));
        for (hipEvent_t& e : g->joined) WLK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        *out = g.release();
        return WLK_OK;
    });
}

int wlk_group_destroy(wlk_group* g) {
    delete g;
    return WLK_OK;
}

int wlk_group_step_pick(wlk_group* g, wlk_session* const* sessions, const int64_t* tokens, const wlk_pick_params* p, int n,
                        int32_t* tokens_out, float* logprobs_out) {
    if (!g || !sessions || !tokens || !p || !tokens_out || !logprobs_out) return fail(WLK_ERR_ARG, "NULL argument");
    if (n < 1 || n > g->max_rows) return fail(WLK_ERR_ARG, "window group: 1..max_rows sessions per step");
    const wlk_dims& D = g->m->D;
    // every session is checked on the host before anything is launched: a refused call has advanced nobody
    for (int r = 0; r < n; ++r) {
        const wlk_session* s = sessions[r];
        if (!s) return fail(WLK_ERR_ARG, "window group: NULL session");
        for (int j = 0; j < r; ++j)
            if (sessions[j] == s) return fail(WLK_ERR_ARG, "window group: a session is listed twice");
        if (s->m != g->m) return fail(WLK_ERR_ARG, "window group: a session of another model");
        if (s->beam != 1) return fail(WLK_ERR_ARG, "window group: only sessions of one row");
        if (tokens[r] < 0 || tokens[r] >= D.n_vocab) return fail(WLK_ERR_ARG, "token id out of range");
        if (!pick_params_ok(p[r], D.n_vocab)) return fail(WLK_ERR_ARG, "rule parameters out of range");
        if (s->engine) return fail(WLK_ERR_STATE, "window group: the session is attached to the batch engine (its steps belong to the engine's loops)");
        if (!s->encoded || s->n_steps < 1) return fail(WLK_ERR_STATE, "window group: step before the session's prefill");
        if (!s->rules_mask) return fail(WLK_ERR_STATE, "window group: step before wlk_rules_set");
        if (s->self_len + 1 > D.n_text_ctx) return fail(WLK_ERR_STATE, "text context exceeded");
    }
    return guarded([&]() {
        std::lock_guard<std::mutex> lk(g->mu);
        WLK_HIP(hipSetDevice(g->m->device));
        GroupBlock* blk = reinterpret_cast<GroupBlock*>(g->pinned);
        int* res = reinterpret_cast<int*>(g->pinned + sizeof(GroupBlock));
        for (int r = 0; r < n; ++r) {
            wlk_session* s = sessions[r];
            blk->rows[r] = next_step_row(s, (int)tokens[r], D.n_audio_ctx);
            blk->pick[r] = PickRowEntry{s->rules_mask, pick_rules_of(p[r])};
            // encode, prefill and an earlier step of the session's own chain have finished before this stream touches its caches
            WLK_HIP(hipEventRecord(g->joined[r], s->stream));
            WLK_HIP(hipStreamWaitEvent(g->stream, g->joined[r], 0));
        }
        const size_t up = offsetof(GroupBlock, pick) + (size_t)n * sizeof(PickRowEntry);
        WLK_HIP(hipMemcpyAsync(g->blk_dev, blk, up, hipMemcpyHostToDevice, g->stream));
        g->enqueue_step(n);
        WLK_HIP(hipMemcpyAsync(res, g->pick_dev, (size_t)8 * n, hipMemcpyDeviceToHost, g->stream));
        WLK_HIP(hipStreamSynchronize(g->stream));
        for (int r = 0; r < n; ++r) {
            wlk_session* s = sessions[r];
            s->self_len += 1;
            s->n_steps += 1;
            s->have_sot = false;
            s->last_rows = 1;
            s->last_ntok = 1;
            tokens_out[r] = res[2 * r];
            std::memcpy(&logprobs_out[r], &res[2 * r + 1], 4);
        }
        g->last_rows = n;
        g->n_steps += 1;
        g->n_rows += (uint64_t)n;
        return WLK_OK;
    });
}

int wlk_group_stats(wlk_group* g, uint64_t* steps, uint64_t* rows) {
    if (!g) return fail(WLK_ERR_ARG, "group is NULL");
    std::lock_guard<std::mutex> lk(g->mu);
    if (steps) *steps = g->n_steps;
    if (rows) *rows = g->n_rows;
    return WLK_OK;
}

int wlk_group_export_logits(wlk_group* g, int row, float* host, uint64_t capacity, uint64_t* n_written) {
    if (!g || !host) return fail(WLK_ERR_ARG, "NULL argument");
    std::lock_guard<std::mutex> lk(g->mu);
    if (row < 0 || row >= g->last_rows) return fail(WLK_ERR_STATE, "window group: no such row in the last step");
    const uint64_t V = (uint64_t)g->m->D.n_vocab;
    if (n_written) *n_written = V;
    if (V > capacity) return fail(WLK_ERR_CAPACITY, "export buffer too small");
    return guarded([&]() {
        WLK_HIP(hipSetDevice(g->m->device));
        WLK_HIP(hipStreamSynchronize(g->stream));
        copy_sync(host, g->logits + (size_t)row * V, V * sizeof(float), hipMemcpyDeviceToHost);
        return WLK_OK;
    });
}

// Tests: rules_pick_rows_kernel on logits rows, rule masks (bit 0 = always suppressed, bit 1 = blank, as wlk_rules_set
// builds them) and parameters given from the host - so that one and the same row can be put through it and through
// wlk_pick_greedy.  Row r uses masks[mask_of_row[r]].
int wlk_diag_pick_rows(const float* logits_host, int n_vocab, const uint8_t* masks_host, int n_masks, const int32_t* mask_of_row,
                       const wlk_pick_params* p, int n, int32_t* tokens_out, float* logprobs_out) {
    if (!logits_host || !masks_host || !mask_of_row || !p || !tokens_out || !logprobs_out) return fail(WLK_ERR_ARG, "NULL argument");
    if (n < 1 || n > kGroupMaxRows || n_masks < 1 || n_masks > kGroupMaxRows || n_vocab < 1) return fail(WLK_ERR_ARG, "pick rows: 1..8 rows and masks");
    for (int r = 0; r < n; ++r)
        if (mask_of_row[r] < 0 || mask_of_row[r] >= n_masks || !pick_params_ok(p[r], n_vocab))
            return fail(WLK_ERR_ARG, "pick rows: mask index or rule parameters out of range");
    return guarded([&]() {
        const size_t V = (size_t)n_vocab;
        float* logits = dev_alloc<float>(V * n);
        unsigned char* masks = dev_alloc<unsigned char>(V * n_masks);
        PickRowEntry* table = reinterpret_cast<PickRowEntry*>(dev_alloc<char>(sizeof(PickRowEntry) * kGroupMaxRows));
        int* out = dev_alloc<int>(2 * kGroupMaxRows);
        auto release = [&] {
            (void)hipFree(logits); (void)hipFree(masks); (void)hipFree(table); (void)hipFree(out);
        };
        try {
            PickRowEntry host[kGroupMaxRows];
            for (int r = 0; r < n; ++r) host[r] = PickRowEntry{masks + V * mask_of_row[r], pick_rules_of(p[r])};
            copy_sync(logits, logits_host, V * n * sizeof(float), hipMemcpyHostToDevice);
            copy_sync(masks, masks_host, V * n_masks, hipMemcpyHostToDevice);
            copy_sync(table, host, sizeof(PickRowEntry) * n, hipMemcpyHostToDevice);
            launch_rules_pick_rows(LaunchCtx{nullptr, nullptr}, logits, n_vocab, n, table, out);
            int res[2 * kGroupMaxRows];
            WLK_HIP(hipStreamSynchronize(nullptr));
            copy_sync(res, out, (size_t)8 * n, hipMemcpyDeviceToHost);
            for (int r = 0; r < n; ++r) {
                tokens_out[r] = res[2 * r];
                std::memcpy(&logprobs_out[r], &res[2 * r + 1], 4);
            }
        } catch (...) {
            release();
            throw;
        }
        release();
        return WLK_OK;
    });
}

}  // extern "C"
