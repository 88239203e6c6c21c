// The decoder chains over a StepRow table (decoder_chain.h): the stacked prefill of several sessions and the single-token
// step of up to 8 rows - embedding, wlk_decoder_layers, read-out - with their workspaces.
#include <algorithm>

#include "common.h"
#include "decoder_chain.h"
#include "internal.h"

using namespace wlk;

// ---- stacked prefills (see decoder_chain.h) -----------------------------------------------------------------------------------
void wlk_prefill_ws_alloc(const wlk_model* m, wlk_prefill_ws& ws, int max_sessions, int session_rows) {
    const wlk_dims& D = m->D;
    const size_t d = D.n_text_state, V = D.n_vocab, H = D.n_text_head;
    ws.cap_session_rows = session_rows;
    ws.cap_rows = max_sessions * ((session_rows + 31) / 32 * 32);
    const size_t R = ws.cap_rows;
    ws.dx = dev_alloc<float>(R * d);
    ws.dh = dev_alloc<float>(R * d);
    ws.dqkv = dev_alloc<float>(R * 3 * d);
    ws.datt = dev_alloc<float>(R * d);
    ws.dq = dev_alloc<float>(R * d);
    ws.dmlp = dev_alloc<float>(R * 4 * d);
    ws.hsel = dev_alloc<float>((size_t)2 * max_sessions * d);
    ws.logits = dev_alloc<float>((size_t)8 * V);
    ws.part = dev_alloc<float>(flash_split_scratch_floats((int)R, (int)H, wlk_session::kFlashSplitsMax));
    ws.rows_dev = reinterpret_cast<StepRow*>(dev_alloc<char>(R * sizeof(StepRow)));
    ws.tiles_dev = reinterpret_cast<StepRow*>(dev_alloc<char>(R / 32 * sizeof(StepRow)));
    ws.ring_row_dev = dev_alloc<int>(R);
    ws.zeros_dev = dev_alloc<int>(R);
    memset_sync(ws.zeros_dev, 0, R * sizeof(int));
    ws.pinned_bytes = R * sizeof(StepRow) + R / 32 * sizeof(StepRow) + R * sizeof(int);
    WLK_HIP(hipHostMalloc(reinterpret_cast<void**>(&ws.pinned), ws.pinned_bytes, hipHostMallocDefault));
}

void wlk_prefill_ws_free(wlk_prefill_ws& ws) {
    void* dev[] = {ws.dx, ws.dh, ws.dqkv, ws.datt, ws.dq, ws.dmlp, ws.hsel, ws.logits, ws.part, ws.rows_dev, ws.tiles_dev,
                   ws.ring_row_dev, ws.zeros_dev};
    for (void* p : dev)
        if (p) (void)hipFree(p);
    if (ws.pinned) (void)hipHostFree(ws.pinned);
    ws = wlk_prefill_ws{};
}

std::string wlk_prefill_precheck(const wlk_prefill_item& it, const wlk_prefill_ws& ws) {
    const wlk_session* s = it.s;
    if (!s || !it.tokens) return "prefill: NULL argument";
    const wlk_dims& D = s->m->D;
    const int P = it.n_tok, d = D.n_text_state;
    if (!s->encoded) return "wlk_decode before wlk_encode";
    if (s->beam != 1 || s->debug || s->prof_on || s->align_raw_scores || s->survey) return "not a plain beam-1 session";
    if (it.sot_index < 0 || it.sot_index >= P) return "sot_index out of range";
    if (P > D.n_text_ctx) return "text context exceeded";
    for (int i = 0; i < P; ++i)
        if (it.tokens[i] < 0 || it.tokens[i] >= D.n_vocab) return "token id out of range";
    const std::string shape = wlk_prefill_shape_check(s->m, P, ws.cap_session_rows);
    if (!shape.empty()) return shape;
    if (!gemv_applicable(8, d)) return "model too wide for the stacked vocabulary projection";
    return std::string();
}

std::string wlk_prefill_shape_check(const wlk_model* m, int P, int cap_session_rows) {
    const wlk_dims& D = m->D;
    const int d = D.n_text_state;
    // the stack runs every GEMM on the k-wave kernel and the cross-attention with key splits: only prompts whose own
    // prefill would make exactly these choices ride in it (bit-identical results either way)
    if (P <= 8 || P > cap_session_rows) return "prompt length outside the stacked range";
    if (!gemm_takes_kwave(P, 3 * d, d) || !gemm_takes_kwave(P, d, d) || !gemm_takes_kwave(P, 4 * d, d) ||
        !gemm_takes_kwave(P, d, 4 * d))
        return "prompt too long for the k-wave GEMMs";
    if (((P + 31) / 32) * D.n_text_head >= 256) return "prompt too long for the key-split cross-attention";
    return std::string();
}

// The stacked chain up to the last layer's output: tables, embedding, the L layers - the flash cross-attention leaves the
// alignment heads' raw scores in rows 0 .. P-1 of each session's score window.  The one statement of it for the stacked
// prefills (wlk_prefill_group: read-out tail behind it) and the stacked alignment pass (wlk_group_find_alignment).
// row0[i] = first stacked row of items[i] in ws.dx; touches no session bookkeeping.
void wlk_prefill_chain(const std::vector<wlk_prefill_item*>& items, const LaunchCtx& c, wlk_prefill_ws& ws,
                       std::vector<int>& row0) {
    wlk_model* m = items[0]->s->m;
    const int d = m->D.n_text_state;
    const int B = (int)items.size();
    // ---- tables: one StepRow per stacked row; a session's rows are padded to whole 32-row tiles with copies of its
    // row 0 (same token, position, destinations: every write of a copy repeats row 0's write with the same value)
    StepRow* rows_h = reinterpret_cast<StepRow*>(ws.pinned);
    std::vector<int> padded(B);
    row0.assign(B, 0);
    int R = 0;
    for (int i = 0; i < B; ++i) {
        row0[i] = R;
        padded[i] = (items[i]->n_tok + 31) / 32 * 32;
        R += padded[i];
    }
    if (R > ws.cap_rows) throw std::length_error("stacked prefill: more rows than the workspace holds");
    StepRow* tiles_h = rows_h + R;
    int* ring_row_h = reinterpret_cast<int*>(tiles_h + R / 32);
    for (int i = 0; i < B; ++i) {
        wlk_session* s = items[i]->s;
        for (int p = 0; p < padded[i]; ++p) {
            const int src = p < items[i]->n_tok ? p : 0;
            StepRow r{};
            r.kcache = s->kcache[s->kv_cur];
            r.vcache = s->vcache[s->kv_cur];
            r.cross_kv = s->cross_kv;
            r.ring = s->ring;
            r.token = (int)items[i]->tokens[src];
            r.offset = src;
            r.ring_row = src;
            rows_h[row0[i] + p] = r;
            ring_row_h[row0[i] + p] = src;
            if (p % 32 == 0) tiles_h[(row0[i] + p) / 32] = r;
        }
    }
    WLK_HIP(hipMemcpyAsync(ws.rows_dev, rows_h, (size_t)R * sizeof(StepRow), hipMemcpyHostToDevice, c.stream));
    WLK_HIP(hipMemcpyAsync(ws.tiles_dev, tiles_h, (size_t)(R / 32) * sizeof(StepRow), hipMemcpyHostToDevice, c.stream));
    WLK_HIP(hipMemcpyAsync(ws.ring_row_dev, ring_row_h, (size_t)R * sizeof(int), hipMemcpyHostToDevice, c.stream));

    // ---- the chain: a session's own prefill (rows > 8) with stacked rows - every GEMM on the k-wave kernel, the
    // cross-attention on the flash kernel with key splits, as wlk_prefill_shape_check promised for each prompt alone
    launch_embed_rows(c, ws.rows_dev, m->w_tok_emb, m->w_dec_pos, ws.dx, R, d);
    wlk_decoder_layers(c, m, dec_ws(ws), R, DecForm::kKwave, DecRowAddr{m, ws.rows_dev, false, nullptr, &ws});
}

void wlk_prefill_group(const std::vector<wlk_prefill_item*>& items, const LaunchCtx& c, wlk_prefill_ws& ws) {
    if (items.empty()) return;
    wlk_model* m = items[0]->s->m;
    const wlk_dims& D = m->D;
    const int d = D.n_text_state, T = D.n_audio_ctx, V = D.n_vocab;
    const int B = (int)items.size();
    std::vector<int> row0;
    wlk_prefill_chain(items, c, ws, row0);
    // ---- per session: the alignment heads' raw scores softmaxed in place; final LayerNorm of the last and the sot row
    for (int i = 0; i < B; ++i) {
        wlk_session* s = items[i]->s;
        const int P = items[i]->n_tok;
        if (m->n_align > 0)
            launch_ring_softmax(c, s->ring, ws.ring_row_dev + row0[i], ws.zeros_dev, m->all_ranks, m->n_align, P, s->ring_rows, 1, T);
        launch_layernorm(c, ws.dx + (size_t)(row0[i] + P - 1) * d, (long)(items[i]->sot_index - (P - 1)) * d, m->w_ln_w, m->w_ln_b,
                         ws.hsel + (size_t)2 * i * d, d, 2, d, "dec_ln_f");
    }
    // ---- vocabulary projection: [last, sot] rows of up to four sessions per pass over the embedding (the <= 8-row
    // weight-streaming kernel, whose per-row arithmetic does not depend on the row count), then out to the sessions
    for (int lo = 0; lo < B; lo += 4) {
        const int nb = std::min(4, B - lo);
        launch_gemv(c, logits_gemm(m, ws.hsel + (size_t)2 * lo * d, 2 * nb, ws.logits), "dec_logits");
        for (int i = 0; i < nb; ++i)
            WLK_HIP(hipMemcpyAsync(items[lo + i]->s->logits_last, ws.logits + (size_t)2 * i * V, (size_t)2 * V * sizeof(float),
                                   hipMemcpyDeviceToDevice, c.stream));
    }
    for (int i = 0; i < B; ++i) {
        wlk_session* s = items[i]->s;
        s->self_len = items[i]->n_tok;
        s->n_steps = 1;
        s->have_sot = true;
        s->prefill_rows = items[i]->n_tok;
        s->last_rows = 1;
        s->last_ntok = items[i]->n_tok;
    }
}

// ---- the step chain ------------------------------------------------------------------------------------------
void wlk_step_ws_alloc(const wlk_model* m, wlk_step_ws& ws) {
    const wlk_dims& D = m->D;
    const size_t R = 8, d = D.n_text_state, V = D.n_vocab;
    ws.x = dev_alloc<float>(R * d);
    ws.qkv = dev_alloc<float>(R * 3 * d);
    ws.att = dev_alloc<float>(R * d);
    ws.q = dev_alloc<float>(R * d);
    ws.mlp = dev_alloc<float>(R * 4 * d);
    ws.logits = dev_alloc<float>(R * V);
    ws.xsplit = dev_alloc<float>(cross_split_scratch_floats(8, D.n_text_head, D.n_audio_ctx));
}

void wlk_step_ws_free(wlk_step_ws& ws) {
    float* fl[] = {ws.x, ws.qkv, ws.att, ws.q, ws.mlp, ws.logits, ws.xsplit};
    for (float* p : fl)
        if (p) (void)hipFree(p);
    ws = wlk_step_ws{};
}

void wlk_enqueue_step_rows(const wlk_model* m, const LaunchCtx& c, const wlk_step_ws& ws, const StepRow* rows_dev, int R,
                           const wlk_step_opts& o) {
    const int d = m->D.n_text_state;
    if (o.block_host) launch_embed_rows_step(c, o.block_host, o.block_dev, m->w_tok_emb, m->w_dec_pos, ws.x, R, d);
    else launch_embed_rows(c, rows_dev, m->w_tok_emb, m->w_dec_pos, ws.x, R, d);
    wlk_decoder_layers(c, m, dec_ws(ws), R, DecForm::kFused, DecRowAddr{m, rows_dev, o.fold_one_row_query, ws.xsplit, nullptr});
    GemmArgs lg = logits_gemm(m, ws.x, R, ws.logits);
    lg.ln_gamma = m->w_ln_w; lg.ln_beta = m->w_ln_b;
    lg.side_align = o.side_align; lg.side_blocks = o.side_blocks; lg.side_zf = o.side_zf;   // fused replay: the rows' z-scores ride here
    launch_gemv(c, lg, "dec_lnf_logits");
}

