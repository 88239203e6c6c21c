// What nllb.hip (one sentence per session) and nllb_batch.hip (up to 8 sentences per launch chain) share: the model
// handle, the per-layer weight pointers, the error convention and argument checks of the wlk_nllb_* entry points, what a
// session and a batch own (NlOwner), the graph slot their steps replay from, and the ONE statement of the encoder and of
// the decoder layer (nl_encoder_layers, nl_decoder_layers).
#pragma once
#include <algorithm>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/wlk_hip.h"
#include "common.h"

namespace wlk {

inline int nl_fail(int code, const std::string& msg) {
    set_last_error(msg);
    return code;
}
template <typename F>
static int nl_guarded(F&& f) {
    try {
        return f();
    } catch (const HipError& e) {
        return nl_fail(WLK_ERR_HIP, e.what());
    } catch (const std::invalid_argument& e) {
        return nl_fail(WLK_ERR_ARG, e.what());
    } catch (const std::exception& e) {
        return nl_fail(WLK_ERR_STATE, e.what());
    }
}

struct NlSlot {
    std::string name;
    uint64_t offset, numel;
};

struct NlLayer {
    const float *ln1w, *ln1b, *qkvw, *qkvb, *outw, *outb, *lnxw, *lnxb, *xqw, *xqb, *xkvw, *xkvb, *xoutw, *xoutb, *ln2w, *ln2b,
        *fc1w, *fc1b, *fc2w, *fc2b;
};

// AlignAtt read-out of an NLLB decoder step (nllb.hip): head mean of the selected heads' softmax rows
// probs [n_align][rows][S], its arg-max over [ctl[0], ctl[1]) and its mass from ctl[2] on; ctl, pos, prob and mass may be
// host-coherent memory.  S <= kSfMaxFrames.
constexpr int kNlMaxAlign = 64;
void launch_nllb_align_readout(const LaunchCtx& ctx, const float* probs, int n_align, int rows, int S, const int* ctl,
                               float* p_out, int* pos, float* prob, float* mass);
// The ragged form of a stacked align step (nllb_batch.hip): row r of n_rows (<= 8) has its own length
// rows[r].content_len (<= stride <= 512) and its own window ctl[3 r .. 3 r + 2] = lo | hi | limit; probs
// [n_align][head_stride / stride][stride], p_out [n_rows][stride].  Nothing is read or written at or past a row's length.
void launch_nllb_align_readout_rows(const LaunchCtx& ctx, const float* probs, int n_align, long head_stride, int stride,
                                    int n_rows, const StepRow* rows, const int* ctl, float* p_out, int* pos, float* prob,
                                    float* mass);

// Draft verification (nllb_batch.hip): the greedy pick of every row of logits [n_rows][n_vocab] in ONE read of the
// row.  A row is split over kNlPickSlices workgroups; each leaves its (value, id) best - order (value descending, id
// ascending), (-inf, INT_MAX) for a slice without elements - in parts [n_rows][kNlPickSlices].  nl_pick_fold (below) folds a
// row's partials; launch_nllb_verify_fold_rows does that for n_rows rows, one lane per row: picks[r] and
// match[r] = (picks[r] == targets[r]) - the diagnostics' route, the accept kernel folds for itself.
constexpr int kNlPickSlices = 32;
struct NlPick {
    float v;
    int i;
};
void launch_nllb_verify_pick_rows(const LaunchCtx& ctx, const float* logits, int n_vocab, int n_rows, NlPick* parts);
void launch_nllb_verify_fold_rows(const LaunchCtx& ctx, const NlPick* parts, int n_rows, const int* targets, int* picks, int* match);

}  // namespace wlk

struct wlk_nllb {
    wlk_nllb_dims D{};
    int device = 0;
    float* arena = nullptr;
    uint64_t arena_floats = 0;
    std::vector<wlk::NlSlot> layout;
    std::map<std::string, const wlk::NlSlot*> index;
    bool finalized = false;
    std::vector<wlk::NlLayer> enc, dec;
    const float *emb = nullptr, *pos = nullptr, *enc_lnw = nullptr, *enc_lnb = nullptr, *dec_lnw = nullptr, *dec_lnb = nullptr;
    const float* P(const std::string& n) const {
        auto it = index.find(n);
        if (it == index.end()) throw std::invalid_argument("unknown packed tensor " + n);
        return arena + it->second->offset;
    }
    ~wlk_nllb() {
        (void)hipSetDevice(device);
        if (arena) (void)hipFree(arena);
    }
};

namespace wlk {

// ---- argument checks of the entry points (host only) ---------------------------------------------------------------------
// every id of ids[n] is a token of the vocabulary and not the padding token; pad_msg is the site's wording of that refusal
inline int nl_check_tokens(const wlk_nllb_dims& D, const int64_t* ids, int n,
                           const char* pad_msg = "padding inside a sequence is not supported") {
    for (int i = 0; i < n; ++i) {
        if (ids[i] < 0 || ids[i] >= D.vocab) return nl_fail(WLK_ERR_ARG, "token id out of range");
        if (ids[i] == D.pad_id) return nl_fail(WLK_ERR_ARG, pad_msg);
    }
    return WLK_OK;
}

// rank [dec_layers][heads]: i for the i-th of the n (layer, head) pairs, -1 for every other head
inline int nl_head_rank(const wlk_nllb_dims& D, const int32_t* pairs, int n, std::vector<int>& rank) {
    rank.assign((size_t)D.dec_layers * D.heads, -1);
    for (int i = 0; i < n; ++i) {
        const int l = pairs[2 * i], h = pairs[2 * i + 1];
        if (l < 0 || l >= D.dec_layers || h < 0 || h >= D.heads) return nl_fail(WLK_ERR_ARG, "alignment head: layer or head out of range");
        if (rank[(size_t)l * D.heads + h] >= 0) return nl_fail(WLK_ERR_ARG, "alignment head: duplicate (layer, head) pair");
        rank[(size_t)l * D.heads + h] = i;
    }
    return WLK_OK;
}

// ---- one recorded single-token step ---------------------------------------------------------------------------------------
// k (the top-k width) and src (a source length) are what the recording carries by value.  A session's cross-attention launch
// carries the source length, so a sentence of another length needs a new recording (round 5: a session that translated a
// 5-token and then a 7-token source replayed the 5-token graph); a batch's graphs read every length from the row table and
// pass src = 0.
struct NlGraphSlot {
    hipGraphExec_t exec = nullptr;
    int k = 0, src = 0;
    void drop() {
        if (exec) { WLK_HIP(hipGraphExecDestroy(exec)); exec = nullptr; }
    }
};

// record `enqueue` into the slot unless it holds a recording of the same k and src, then replay it and wait; true if it recorded
template <typename F>
bool nl_replay(hipStream_t stream, NlGraphSlot& g, int k, int src, F&& enqueue) {
    const bool record = !g.exec || g.k != k || g.src != src;
    if (record) {
        g.drop();
        capture_step_graph(stream, g.exec, enqueue);
        g.k = k;
        g.src = src;
    }
    WLK_HIP(hipGraphLaunch(g.exec, stream));
    WLK_HIP(hipStreamSynchronize(stream));
    return record;
}

// ---- what a session (nllb.hip) and a batch (nllb_batch.hip) own ------------------------------------------------------------
struct NlOwner {
    wlk_nllb* m = nullptr;
    hipStream_t stream = nullptr;
    std::vector<void*> owned, owned_host;
    std::vector<NlGraphSlot> graphs;       // the derived struct says which slot is which
    explicit NlOwner(size_t n_graphs) : graphs(n_graphs) {}
    NlOwner(const NlOwner&) = delete;
    NlOwner& operator=(const NlOwner&) = delete;
    template <typename T>
    T* alloc(size_t n) {
        void* p = nullptr;
        WLK_HIP(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
        owned.push_back(p);
        return static_cast<T*>(p);
    }
    // pinned + mapped host block of n elements, zeroed: *host for the CPU, *dev the same block as the device sees it
    template <typename T>
    void mapped(size_t n, T** host, T** dev) {
        void* p = nullptr;
        WLK_HIP(hipHostMalloc(&p, n * sizeof(T), hipHostMallocMapped));
        owned_host.push_back(p);
        std::memset(p, 0, n * sizeof(T));
        WLK_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(dev), p, 0));
        *host = static_cast<T*>(p);
    }
    LaunchCtx ctx() const { return LaunchCtx{stream, nullptr}; }
    ~NlOwner() {                 // also the clean-up of a half-built owner (an allocation that threw in *_create)
        if (m) (void)hipSetDevice(m->device);
        if (stream) (void)hipStreamSynchronize(stream);
        for (void* p : owned) (void)hipFree(p);
        for (auto& g : graphs) if (g.exec) (void)hipGraphExecDestroy(g.exec);
        for (void* p : owned_host) (void)hipHostFree(p);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// ---- launcher compositions ---------------------------------------------------------------------------------------------
inline GemmArgs nl_gemm(const float* A, long lda, const float* W, const float* b, float* C, long ldc, int M, int N, int K, int flags,
                        const float* R = nullptr, long ldr = 0, float scale = 1.f, int scale_cols = 0) {
    GemmArgs g;
    g.A = A; g.lda = lda; g.W = W; g.bias = b; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
    g.flags = flags; g.R = R; g.ldr = ldr; g.scale = scale; g.scale_cols = scale_cols;
    return g;
}

// the q columns of a q | k | v or q projection carry 64^-0.5 (exact)
constexpr float kNlQScale = 0.125f;

// C = g(LayerNorm(x)), the two projection forms of a decoder chain.  x has row stride g.lda; g.A is not read.
//   fused    the LayerNorm is folded into the weight-streaming GEMV, and so is the KV rider the caller put into g
//   unfused  LayerNorm kernel into h [M][K], then launch_linear from h; a rider in g is dropped (the caller appends)
inline void nl_ln_linear(const LaunchCtx& c, bool fused, const float* x, const float* gamma, const float* beta, float* h, GemmArgs g,
                         const char* tag_fused, const char* tag_ln, const char* tag_linear) {
    if (fused) {
        g.A = x; g.ln_gamma = gamma; g.ln_beta = beta;
        launch_gemv(c, g, tag_fused);
        return;
    }
    launch_layernorm(c, x, g.lda, gamma, beta, h, g.K, g.M, g.K, tag_ln);
    g.A = h; g.lda = g.K;
    g.kcache = g.vcache = nullptr; g.kv_pos = nullptr; g.kv_rows = nullptr; g.kv_d = g.kv_ctx = 0; g.kv_layer_off = 0;
    launch_linear(c, g, tag_linear);
}

inline void nl_ffn(const LaunchCtx& c, const NlLayer& L, bool fused, float* x, float* h, float* wide, int R, int d, int f) {
    nl_ln_linear(c, fused, x, L.ln2w, L.ln2b, h, nl_gemm(nullptr, d, L.fc1w, L.fc1b, wide, f, R, f, d, kGemmRelu), "nllb_ln2_fc1",
                 "nllb_ln2", "nllb_fc1");
    launch_linear(c, nl_gemm(wide, f, L.fc2w, L.fc2b, x, d, R, d, f, kGemmResidual, x, d), "nllb_fc2");
}

// Encoder layers, final LayerNorm and every decoder layer's cross K/V ([S][dec_layers][k | v]) over S embedded rows in ex.
// seg says which rows attend to which: n_seg = 0 and T = S for one sentence, the segments and T = the longest for a stack.
inline void nl_encoder_layers(const LaunchCtx& c, const wlk_nllb* m, float* ex, float* eh, float* eqkv, float* eatt, float* ewide,
                              float* enc_out, float* cross_kv, int S, const SfAttnArgs& seg) {
    const wlk_nllb_dims& D = m->D;
    const int d = D.d_model;
    SfAttnArgs a = seg;
    a.q = eqkv; a.k = eqkv + d; a.v = eqkv + 2 * d; a.ldq = a.ldk = a.ldv = 3 * d;
    a.out = eatt; a.ldo = d; a.n_head = D.heads; a.dh = 64; a.scale = 1.f;
    for (int l = 0; l < D.enc_layers; ++l) {
        const NlLayer& L = m->enc[l];
        nl_ln_linear(c, false, ex, L.ln1w, L.ln1b, eh, nl_gemm(nullptr, d, L.qkvw, L.qkvb, eqkv, 3 * d, S, 3 * d, d, kGemmScaleCols,
                                                               nullptr, 0, kNlQScale, d), nullptr, "nllb_ln1", "nllb_enc_qkv");
        launch_sf_attention(c, a);
        launch_linear(c, nl_gemm(eatt, d, L.outw, L.outb, ex, d, S, d, d, kGemmResidual, ex, d), "nllb_enc_out");
        nl_ffn(c, L, false, ex, eh, ewide, S, d, D.ffn);
    }
    launch_layernorm(c, ex, d, m->enc_lnw, m->enc_lnb, enc_out, d, S, d, "nllb_enc_ln");
    const long ld = (long)D.dec_layers * 2 * d;
    for (int l = 0; l < D.dec_layers; ++l)
        launch_linear(c, nl_gemm(enc_out, d, m->dec[l].xkvw, m->dec[l].xkvb, cross_kv + (size_t)l * 2 * d, ld, S, 2 * d, d, 0), "nllb_xkv");
}

// the activation buffers of a decoder chain, R rows each: x [d] (the residual stream), h [d] (LayerNorm output; null in a
// fused-only workspace), qkv [3 d], att [d], q [d], wide [ffn]
struct NlDecWs {
    float *x, *h, *qkv, *att, *q, *wide;
};

// The decoder layers over the R rows in ws.x - the ONE statement of the eight steps.  Two independent axes:
//   fused  the projection form (nl_ln_linear): single-token steps fold LayerNorm and the cache append into the GEMV
//   Addr   how the caches and the source are reached: one session's dense caches + offset_dev (nllb.hip's NlSessionAddr) or a
//          StepRow table (nllb_batch.hip's NlRowsAddr).  Addr has
//            void kv_rider(GemmArgs& g, int l) const                                    the cache append riding in the qkv GEMV
//            void append(const LaunchCtx&, const float* qkv, int l) const               ... or launched behind the projection
//            void self_attention(const LaunchCtx&, const float* qkv, float* att, int l) const
//            void cross_attention(const LaunchCtx&, const float* q, float* att, int l) const
template <typename Addr>
void nl_decoder_layers(const LaunchCtx& c, const wlk_nllb* m, const NlDecWs& ws, int R, bool fused, const Addr& addr) {
    const wlk_nllb_dims& D = m->D;
    const int d = D.d_model;
    for (int l = 0; l < D.dec_layers; ++l) {
        const NlLayer& L = m->dec[l];
        GemmArgs qkv = nl_gemm(nullptr, d, L.qkvw, L.qkvb, ws.qkv, 3 * d, R, 3 * d, d, kGemmScaleCols, nullptr, 0, kNlQScale, d);
        addr.kv_rider(qkv, l);
        nl_ln_linear(c, fused, ws.x, L.ln1w, L.ln1b, ws.h, qkv, "nllb_ln1_qkv_kv", "nllb_ln1", "nllb_dec_qkv");
        if (!fused) addr.append(c, ws.qkv, l);
        addr.self_attention(c, ws.qkv, ws.att, l);
        launch_linear(c, nl_gemm(ws.att, d, L.outw, L.outb, ws.x, d, R, d, d, kGemmResidual, ws.x, d), "nllb_dec_out");
        nl_ln_linear(c, fused, ws.x, L.lnxw, L.lnxb, ws.h, nl_gemm(nullptr, d, L.xqw, L.xqb, ws.q, d, R, d, d, kGemmScaleCols, nullptr, 0,
                                                                   kNlQScale, d), "nllb_lnx_xq", "nllb_lnx", "nllb_dec_xq");
        addr.cross_attention(c, ws.q, ws.att, l);
        launch_linear(c, nl_gemm(ws.att, d, L.xoutw, L.xoutb, ws.x, d, R, d, d, kGemmResidual, ws.x, d), "nllb_dec_xout");
        nl_ffn(c, L, fused, ws.x, ws.h, ws.wide, R, d, D.ffn);
    }
}

// final LayerNorm + tied vocabulary projection of the last of n_tok fed positions of each of `rows` rows of x: folded into
// the vocabulary GEMV (fused: n_tok == 1), or LayerNorm with row stride n_tok d into hsel, then launch_linear
inline void nl_logits(const LaunchCtx& c, const wlk_nllb* m, bool fused, const float* x, int rows, int n_tok, float* hsel,
                      float* logits) {
    const wlk_nllb_dims& D = m->D;
    const int d = D.d_model;
    nl_ln_linear(c, fused, x + (size_t)(n_tok - 1) * d, m->dec_lnw, m->dec_lnb, hsel,
                 nl_gemm(nullptr, (long)n_tok * d, m->emb, nullptr, logits, D.vocab, rows, D.vocab, d, 0), "nllb_lnf_logits",
                 "nllb_dec_ln", "nllb_logits");
}

}  // namespace wlk
