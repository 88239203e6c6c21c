// The Whisper decoder layers - self-attention, cross-attention, the MLP and their projections - stated ONCE
// (wlk_decoder_layers), and the chains of decoder_chain.hip that run them over a StepRow table.
#pragma once
#include <string>
#include <vector>

#include "common.h"
#include "internal.h"

// ---- stacked prefills (the engine's prefill lane, the window group's alignment pass) -----------------------------------
// Workspace of one stacked prefill chain: activations of all stacked rows, the row / tile tables, read-out staging.
struct wlk_prefill_ws {
    int cap_rows = 0;             // stacked rows (each session padded to whole 32-row query tiles) the buffers hold
    int cap_session_rows = 0;     // longest prompt of one session taken into a stack
    float *dx = nullptr, *dh = nullptr, *dqkv = nullptr, *datt = nullptr, *dq = nullptr, *dmlp = nullptr, *hsel = nullptr,
          *logits = nullptr, *part = nullptr;
    wlk::StepRow *rows_dev = nullptr, *tiles_dev = nullptr;
    int *ring_row_dev = nullptr, *zeros_dev = nullptr;
    char* pinned = nullptr;       // host staging of the tables
    size_t pinned_bytes = 0;
};
struct wlk_prefill_item {
    wlk_session* s = nullptr;
    const int64_t* tokens = nullptr;
    int n_tok = 0, sot_index = 0;
    int rc = 0;
    std::string err;
};
// The prefills (first decoder pass of an infer: all prompt tokens at once) of several beam-1 sessions of one model as
// ONE launch chain on c.stream: rows of all sessions stacked, session pointers per row and per query tile.
// Every row goes through the kernels and the arithmetic of a prefill of its session alone (wlk_decode, first = 1), so the
// results are bit-identical to it.  wlk_prefill_precheck: empty = this request can ride in a stack (otherwise the
// caller runs wlk_decode).  Leaves each session as wlk_decode(first = 1) leaves it; throws on launch failures.
std::string wlk_prefill_precheck(const wlk_prefill_item& it, const wlk_prefill_ws& ws);
void wlk_prefill_group(const std::vector<wlk_prefill_item*>& items, const wlk::LaunchCtx& c, wlk_prefill_ws& ws);
void wlk_prefill_chain(const std::vector<wlk_prefill_item*>& items, const wlk::LaunchCtx& c, wlk_prefill_ws& ws,
                       std::vector<int>& row0);
// the shape conditions of wlk_prefill_precheck alone: empty = a prompt of P tokens can ride in a stacked chain of model m
std::string wlk_prefill_shape_check(const wlk_model* m, int P, int cap_session_rows);
void wlk_prefill_ws_alloc(const wlk_model* m, wlk_prefill_ws& ws, int max_sessions, int session_rows);
void wlk_prefill_ws_free(wlk_prefill_ws& ws);

// ---- the single-token step of up to 8 rows over a StepRow table: the batch engine's steps and the window group's --------
// Activations of one such step, 8 rows each (xsplit: the split cross-attention's scratch).
struct wlk_step_ws {
    float *x = nullptr, *qkv = nullptr, *att = nullptr, *q = nullptr, *mlp = nullptr, *logits = nullptr, *xsplit = nullptr;
};
void wlk_step_ws_alloc(const wlk_model* m, wlk_step_ws& ws);
void wlk_step_ws_free(wlk_step_ws& ws);
// what a caller's chain may differ in
struct wlk_step_opts {
    // embedding: the tokens and offsets come out of the host-coherent block `block_host` (its device-side address), which the
    // first kernel also copies into `block_dev`, whose `rows` is then the table (launch_embed_rows_step); nullptr = the table
    const wlk::EngineBlock* block_host = nullptr;
    wlk::EngineBlock* block_dev = nullptr;
    // riders of the vocabulary GEMV (GemmArgs::side_align): the rows' z-scores of a fused replay
    const wlk::AlignArgs* side_align = nullptr;
    int side_blocks = 0, side_zf = 0;
    // a step of ONE row folds the cross-attention's query projection into the attention kernel where that kernel can
    bool fold_one_row_query = false;
};
// embed .. logits of R rows on c.stream: the one statement of the chain, whoever takes the step
void wlk_enqueue_step_rows(const wlk_model* m, const wlk::LaunchCtx& c, const wlk_step_ws& ws, const wlk::StepRow* rows_dev, int R,
                           const wlk_step_opts& o = wlk_step_opts{});

namespace wlk {

// the activation buffers of a chain, R rows each: x [d] (the residual stream), h [d] (LayerNorm output; null where only fused
// steps run), qkv [3 d], att [d], q [d], mlp [4 d]
struct DecWs { float *x, *h, *qkv, *att, *q, *mlp; };
inline DecWs dec_ws(const wlk_session* s) { return DecWs{s->dx, s->dh, s->dqkv, s->datt, s->dq, s->dmlp}; }
inline DecWs dec_ws(const wlk_prefill_ws& w) { return DecWs{w.dx, w.dh, w.dqkv, w.datt, w.dq, w.dmlp}; }
inline DecWs dec_ws(const wlk_step_ws& w) { return DecWs{w.x, nullptr, w.qkv, w.att, w.q, w.mlp}; }

// the vocabulary projection of M rows of A ([M][d]) into logits [M][n_vocab]
inline GemmArgs logits_gemm(const wlk_model* m, const float* A, int M, float* logits) {
    GemmArgs lg;
    lg.A = A; lg.lda = m->D.n_text_state; lg.W = m->w_tok_emb; lg.C = logits; lg.ldc = m->D.n_vocab; lg.M = M; lg.N = m->D.n_vocab;
    lg.K = m->D.n_text_state;
    return lg;
}

// how a projection behind a LayerNorm is launched
enum class DecForm {
    kFused,    // LayerNorm and the KV rider folded into launch_gemv (single-token steps)
    kLinear,   // launch_layernorm, then launch_linear (a session's prefill)
    kKwave     // launch_layernorm, then the k-wave GEMM whatever the shape (the stack: every row keeps its solo arithmetic)
};
enum class CrossRoute { kFlash, kSplit, kPlain };

// One session's dense caches [L][beam][ctx][d], offset scalar and score window; n_tok fed positions for each of n_rows beams.
// ancestry: the self-attention reads through the ancestry table, which the caller has brought up to date.
struct DecSessionAddr {
    static constexpr bool kGemvOnly = false;
    const wlk_session* s;
    int n_rows, n_tok;
    bool ancestry = false;
    int d() const { return s->m->D.n_text_state; }
    int ctx_len() const { return s->m->D.n_text_ctx; }
    float* kc(int l) const { return s->kcache[s->kv_cur] + (size_t)l * s->beam * ctx_len() * d(); }
    float* vc(int l) const { return s->vcache[s->kv_cur] + (size_t)l * s->beam * ctx_len() * d(); }
    // find_alignment and the head survey: the flash kernel whatever the row count, its q never folded, no window softmax
    bool raw_pass() const { return s->align_raw_scores || s->survey; }
    void kv_rider(GemmArgs& g, int l) const {
        g.kcache = kc(l); g.vcache = vc(l); g.kv_pos = s->d_offset; g.kv_d = d(); g.kv_ctx = ctx_len(); g.kv_ntok = n_tok;
    }
    void append(const LaunchCtx& c, const float* qkv, int l, int) const {
        launch_kv_append(c, qkv, kc(l), vc(l), n_rows, n_tok, s->d_offset, d(), ctx_len());
    }
    void self_attention(const LaunchCtx& c, const float* qkv, float* att, int l, int) const {
        const int H = s->m->D.n_text_head;
        if (ancestry) launch_decoder_self_attention_anc(c, qkv, kc(l), vc(l), s->anc, att, n_rows, s->d_offset, d(), H, ctx_len());
        else launch_decoder_self_attention(c, qkv, kc(l), vc(l), att, n_rows, n_tok, s->d_offset, d(), H, ctx_len());
    }
    // head survey: every layer's queries are kept
    float* query_out(float* q, int l, int R) const { return s->survey ? s->survey_buf + (size_t)l * R * d() : q; }
    // one row: the fold saves a launch; several rows would each re-stream Wq.  It leaves no q behind, so it must never meet
    // the flash kernel, which reads q: a raw pass is excluded here, not merely "never fed with R == 1 today"
    bool folds_query(bool fused, int R) const { return fused && R == 1 && !s->debug && !raw_pass(); }
    CrossRoute cross_route(int R) const {
        if ((R > 8 || raw_pass()) && !s->debug) return CrossRoute::kFlash;   // prefill: 32 query rows share every K/V tile
        return R <= 8 && !s->debug ? CrossRoute::kSplit : CrossRoute::kPlain;
    }
    // beam-1 steps: the merge of the key splits is the A-operand load of the out projection
    bool merges_in_xout(bool fused, int R) const { return fused && R == 1; }
    float* xsplit() const { return s->xsplit; }
    void flash(FlashArgs& fa, int l, int R) const {
        fa.k = s->cross_kv + (size_t)l * 2 * d(); fa.v = fa.k + d();
        fa.ring = s->ring; fa.ring_row = s->ring_row; fa.beam_of_row = s->beam_of_row; fa.ring_rows = s->ring_rows; fa.n_beam = s->beam;
        if (((R + 31) / 32) * fa.n_head >= 256) return;
        fa.k_splits = wlk_session::flash_splits();      // few query tiles: spread the 1500 keys over more workgroups
        flash_split_partition(fa, s->fsplit, s->max_rows);
    }
    void cross(CrossAttnArgs& ca, int l) const {
        ca.k = s->cross_kv + (size_t)l * 2 * d(); ca.v = ca.k + d();
        ca.ring = s->ring; ca.ring_row = s->ring_row; ca.beam_of_row = s->beam_of_row; ca.ring_rows = s->ring_rows; ca.n_beam = s->beam;
        ca.qk_debug = s->debug ? s->qk_debug + (size_t)l * s->max_rows * ca.n_head * ca.T : nullptr;
    }
};

// A StepRow per row: caches, cross K|V, score window and position of beam-1 sessions, row by row.  A step (<= 8 rows) takes
// the split cross-attention with its merge; a stack (`stack` set: whole 32-row query tiles, a StepRow per tile) the flash
// kernel with key splits, its window rows in ring_row_dev and zeros_dev for the beams.
struct DecRowAddr {
    static constexpr bool kGemvOnly = true;
    const wlk_model* m;
    const StepRow* rows;
    bool fold_one_row_query;
    float* xsplit_buf;
    const wlk_prefill_ws* stack;
    int d() const { return m->D.n_text_state; }
    int ctx_len() const { return m->D.n_text_ctx; }
    long cache_off(int l) const { return (long)l * ctx_len() * d(); }       // beam 1: [L][ctx][d]
    void kv_rider(GemmArgs& g, int l) const { g.kv_rows = rows; g.kv_layer_off = cache_off(l); g.kv_d = d(); g.kv_ctx = ctx_len(); }
    void append(const LaunchCtx& c, const float* qkv, int l, int R) const { launch_kv_append_rows(c, qkv, rows, cache_off(l), R, d()); }
    void self_attention(const LaunchCtx& c, const float* qkv, float* att, int l, int R) const {
        launch_decoder_self_attention_rows(c, qkv, rows, cache_off(l), att, R, d(), m->D.n_text_head, ctx_len());
    }
    float* query_out(float* q, int, int) const { return q; }
    // several rows keep the query projection as ONE multi-row GEMV (weights streamed once for all rows): folded into the
    // split cross-attention every row's 64 workgroups would stream Wq again (19 us per launch at 8 streams,
    // profiles/r04_trace8_busy.txt) - the fold only pays for a single row, where it saves a launch
    bool folds_query(bool, int R) const { return fold_one_row_query && R == 1; }
    CrossRoute cross_route(int) const { return stack ? CrossRoute::kFlash : CrossRoute::kSplit; }
    bool merges_in_xout(bool, int) const { return false; }
    float* xsplit() const { return xsplit_buf; }
    void flash(FlashArgs& fa, int l, int R) const {
        fa.tile_rows = stack->tiles_dev; fa.tile_kv_off = (long)l * 2 * d(); fa.tile_v_off = d();
        fa.ring_row = stack->ring_row_dev; fa.beam_of_row = stack->zeros_dev; fa.ring_rows = ctx_len() + kAlignWindow; fa.n_beam = 1;
        fa.k_splits = wlk_session::flash_splits();
        flash_split_partition(fa, stack->part, R);
    }
    void cross(CrossAttnArgs& ca, int l) const {
        ca.ring_rows = ctx_len() + kAlignWindow; ca.n_beam = 1; ca.step_rows = rows; ca.kv_off = (long)l * 2 * d();
    }
};

// The L decoder layers over the R rows in ws.x, on two independent axes: `form`, how a projection is launched, and Addr, where
// the K/V, the score window and the rows' positions live.  The flash route leaves the alignment heads' RAW scores in the
// window: the caller softmaxes them (or not) behind the last layer.
template <typename Addr>
void wlk_decoder_layers(const LaunchCtx& c, const wlk_model* m, const DecWs& ws, int R, DecForm form, const Addr& addr) {
    const wlk_dims& D = m->D;
    const int d = D.n_text_state, T = D.n_audio_ctx, H = D.n_text_head;
    const float scale = qk_scale();
    const bool fused = form == DecForm::kFused;
    // C[R][N] = A[R][K] W^T + bias, both operands dense; the first scale_cols columns carry `scale`
    auto gemm = [R, scale](const float* A, int K, const float* W, const float* bias, float* C, int N, int flags = 0, int scale_cols = 0) {
        GemmArgs g;
        g.A = A; g.lda = K; g.W = W; g.bias = bias; g.C = C; g.ldc = N; g.M = R; g.N = N; g.K = K; g.flags = flags;
        if (scale_cols) { g.scale = scale; g.scale_cols = scale_cols; }
        return g;
    };
    auto project = [&](GemmArgs g, const char* tag) {       // <= 8 rows: launch_linear takes the weight-streaming GEMV
        if (Addr::kGemvOnly && fused) return launch_gemv(c, g, tag);      // a row step refuses what the GEMV cannot take
        if (form != DecForm::kKwave) return launch_linear(c, g, tag);
        g.force_kwave = true; g.ldr = g.ldc;
        launch_gemm(c, g, tag);
    };
    auto residual = [&](GemmArgs g, const char* tag) {      // x += ...
        g.flags = kGemmResidual; g.R = ws.x; g.ldr = d;
        project(g, tag);
    };
    // C = g(LayerNorm(x)): folded into the GEMV with whatever rider g carries, or its own kernel in front of the projection
    // (folding it into the MFMA GEMM's tile staging was measured slower: every workgroup re-derives the row statistics)
    auto ln_project = [&](bool fold, const float* gamma, const float* beta, GemmArgs g, const char* t_fold, const char* t_ln,
                          const char* tag) {
        g.A = fold ? ws.x : ws.h;
        if (fold) { g.ln_gamma = gamma; g.ln_beta = beta; return launch_gemv(c, g, t_fold); }
        launch_layernorm(c, ws.x, d, gamma, beta, ws.h, d, R, d, t_ln);
        project(g, tag);
    };
    for (int l = 0; l < D.n_text_layer; ++l) {
        const LayerW& L = m->dec_layers[l];
        GemmArgs g = gemm(nullptr, d, L.qkvw, L.qkvb, ws.qkv, 3 * d, kGemmScaleCols, 2 * d);
        // k and v also land in the caches: a rider of the GEMV or of a session prompt's k-wave GEMM, else a launch of its own
        const bool rider = fused || (form == DecForm::kLinear && !gemv_applicable(R, d) && gemm_takes_kwave(R, 3 * d, d));
        if (rider) addr.kv_rider(g, l);
        ln_project(fused, L.ln1w, L.ln1b, g, "dec_ln1_qkv_kv", "dec_ln1", "dec_qkv");
        if (!rider) addr.append(c, ws.qkv, l, R);
        addr.self_attention(c, ws.qkv, ws.att, l, R);
        residual(gemm(ws.att, d, L.outw, L.outb, ws.x, d), "dec_out");
        const GemmArgs q = gemm(nullptr, d, L.xqw, L.xqb, addr.query_out(ws.q, l, R), d, kGemmScaleCols, d);
        // the split cross-attention kernel derives its head's query values itself (same arithmetic): one launch less
        const bool fold_xq = addr.folds_query(fused, R) && cross_split_folds_query(d);
        if (!fold_xq) ln_project(fused, L.lnxw, L.lnxb, q, "dec_lnx_xq", "dec_lnx", "dec_xq");
        const int* ranks = m->n_align > 0 ? m->head_rank + (size_t)l * H : nullptr;
        const CrossRoute route = addr.cross_route(R);
        GemmArgs xo = gemm(ws.att, d, L.xoutw, L.xoutb, ws.x, d);
        if (route == CrossRoute::kFlash) {
            if (fold_xq) throw std::logic_error("decode: the folded query projection left no q for the flash kernel");
            FlashArgs fa;
            fa.q = q.C; fa.ldq = d; fa.ldkv = (long)D.n_text_layer * 2 * d;
            fa.out = ws.att; fa.ldo = d; fa.Tq = R; fa.Tk = T; fa.n_head = H; fa.head_rank = ranks;
            addr.flash(fa, l, R);
            launch_prefill_cross_attention(c, fa);
        } else {
            CrossAttnArgs ca{};
            ca.q = ws.q; ca.ldkv = (long)D.n_text_layer * 2 * d; ca.out = ws.att;
            ca.rows = R; ca.d = d; ca.n_head = H; ca.T = T; ca.head_rank = ranks;
            addr.cross(ca, l);
            if (fold_xq) {
                ca.xq_x = ws.x; ca.xq_w = L.xqw; ca.xq_b = L.xqb; ca.xq_gamma = L.lnxw; ca.xq_beta = L.lnxb; ca.xq_scale = scale;
            }
            const CrossSplitScratch p = cross_split_partition(addr.xsplit(), 8, H, T);
            const bool merged_xout = route == CrossRoute::kSplit && addr.merges_in_xout(fused, R) && gemv1_folds_merge(d);
            if (route == CrossRoute::kSplit) launch_decoder_cross_attention_split(c, ca, p.scores, p.pm, p.pl, p.po, !merged_xout);
            else launch_decoder_cross_attention(c, ca);
            if (merged_xout) {      // the out projection takes the split form as its operand
                xo.mg_pm = p.pm; xo.mg_pl = p.pl; xo.mg_po = p.po; xo.mg_scores = p.scores; xo.mg_heads = H; xo.mg_T = T;
                xo.mg_head_rank = ranks; xo.mg_side_heads = m->layer_heads + (size_t)l * H;
                xo.mg_ring = ca.ring; xo.mg_ring_row = ca.ring_row; xo.mg_beam_of_row = ca.beam_of_row;
                xo.mg_ring_rows = ca.ring_rows; xo.mg_n_beam = ca.n_beam; xo.mg_side_blocks = ranks ? m->layer_rank_count[l] : 0;
            }
        }
        residual(xo, "dec_xout");
        // the MLP folds its LayerNorm wherever the GEMV takes the rows, a short prompt's included
        ln_project(fused || gemv_applicable(R, d), L.ln2w, L.ln2b, gemm(nullptr, d, L.fc1w, L.fc1b, ws.mlp, 4 * d, kGemmGelu),
                   "dec_ln2_fc1", "dec_ln2", "dec_fc1");
        residual(gemm(ws.mlp, 4 * d, L.fc2w, L.fc2b, ws.x, d), "dec_fc2");
    }
}

}  // namespace wlk
