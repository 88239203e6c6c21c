// NLLB-200 (M2M-100 architecture) translation model of config 5: the network the reference loads
// through the third-party `nllw` package (whisperlivekit/core.py:320-329) - not in the reference tree.  The arithmetic
// restated here is the published M2M-100 of `transformers` (models/m2m_100/modeling_m2m_100.py, 5.15.0 in this image),
// which is what pins it (tests/golden/nllb_kat.npz):
//
//   embed(ids)   = shared[ids] * sqrt(d_model) + sinusoid[position], position = index + padding_idx + 1 (no padding
//                  inside a sequence: one sentence per call)
//   encoder      = N x { x += Wo . MHA(LN(x)) ; x += W2 . relu(W1 . LN(x)) } ; LN          (pre-LN, biases everywhere)
//   decoder      = N x { x += self-MHA(LN(x)) with KV cache ; x += cross-MHA(LN(x), encoder) ; x += FFN(LN(x)) } ; LN
//   logits       = LN(x) . shared^T                                                         (tied, no bias)
//   attention    = softmax((q * dh^-0.5) . k^T) . v, heads of 64
//
// Everything is a composition of the launchers the Whisper / Sortformer paths already use (MFMA GEMM with bias / ReLU /
// residual / column-scale epilogues, weight-streaming GEMV for the single-token steps, LayerNorm, the LDS-score
// attention for the short non-causal encoder, the KV-cache self-attention and the key-parallel cross-attention of the
// Whisper decoder, log-softmax + top-k): one small kernel is new (token + position embedding).  fp32 throughout.
//
// AlignAtt streaming translation (opt-in per session): the single-token step can keep the softmax rows of chosen
// cross-attention heads (the ring fields of CrossAttnArgs, as the Whisper decoder does) and read off, in one more kernel
// (nllb_align_readout_kernel), which source position the step leans on; wlk_nllb_generate_alignatt is the decoding loop.
#include <climits>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/wlk_hip.h"
#include "common.h"
#include "nllb_internal.h"
#include "wave_ops.h"

namespace wlk {

static std::vector<NlSlot> nl_layout(const wlk_nllb_dims& D, uint64_t* total) {
    std::vector<NlSlot> v;
    uint64_t off = 0;
    auto add = [&](const std::string& n, uint64_t numel) {
        v.push_back({n, off, numel});
        off += (numel + 63) / 64 * 64;
    };
    const uint64_t d = D.d_model, f = D.ffn;
    add("shared.emb", (uint64_t)D.vocab * d);
    add("pos.table", (uint64_t)D.n_positions * d);
    auto block = [&](const std::string& p, bool cross) {
        add(p + "ln1.w", d); add(p + "ln1.b", d);
        add(p + "qkv.w", 3 * d * d); add(p + "qkv.b", 3 * d);           // rows: q | k | v
        add(p + "out.w", d * d); add(p + "out.b", d);
        if (cross) {
            add(p + "lnx.w", d); add(p + "lnx.b", d);
            add(p + "xq.w", d * d); add(p + "xq.b", d);
            add(p + "xkv.w", 2 * d * d); add(p + "xkv.b", 2 * d);       // rows: k | v
            add(p + "xout.w", d * d); add(p + "xout.b", d);
        }
        add(p + "ln2.w", d); add(p + "ln2.b", d);
        add(p + "fc1.w", f * d); add(p + "fc1.b", f);
        add(p + "fc2.w", d * f); add(p + "fc2.b", d);
    };
    for (int i = 0; i < D.enc_layers; ++i) block("enc." + std::to_string(i) + ".", false);
    add("enc.ln.w", d); add("enc.ln.b", d);
    for (int i = 0; i < D.dec_layers; ++i) block("dec." + std::to_string(i) + ".", true);
    add("dec.ln.w", d); add("dec.ln.b", d);
    if (total) *total = off;
    return v;
}

static int nl_check_dims(const wlk_nllb_dims* d) {
    if (!d) return nl_fail(WLK_ERR_ARG, "dims is NULL");
    if (d->vocab < 8 || d->d_model < 64 || d->heads < 1 || d->d_model != 64 * d->heads)
        return nl_fail(WLK_ERR_ARG, "NLLB: d_model must be 64 x heads (heads of 64, as in every released NLLB / M2M-100)");
    if (d->d_model % 4 || d->ffn % 4 || d->ffn < 4 || d->enc_layers < 1 || d->dec_layers < 1)
        return nl_fail(WLK_ERR_ARG, "NLLB: bad layer sizes");
    if (d->max_src < 1 || d->max_src > kSfMaxFrames) return nl_fail(WLK_ERR_ARG, "NLLB: max_src must be 1..512 tokens");
    if (d->max_tgt < 2 || d->max_tgt > 512) return nl_fail(WLK_ERR_ARG, "NLLB: max_tgt must be 2..512 tokens");
    if (d->pad_id < 0 || d->pad_id >= d->vocab) return nl_fail(WLK_ERR_ARG, "NLLB: pad_id out of range");
    if (d->n_positions < std::max(d->max_src, d->max_tgt) + d->pad_id + 1)
        return nl_fail(WLK_ERR_ARG, "NLLB: the position table must cover max(max_src, max_tgt) + pad_id + 1 rows");
    return WLK_OK;
}

// x[r][:] = emb[tokens[r]][:] * scale + pos[pos0 + *offset + (r % n_tok)][:]
__global__ __launch_bounds__(256) void nllb_embed_kernel(const int* __restrict__ tokens, const float* __restrict__ emb,
                                                         const float* __restrict__ pos, float scale, int pos0,
                                                         const int* __restrict__ offset, int n_tok, int d,
                                                         float* __restrict__ x) {
    const int r = blockIdx.x;
    const float* e = emb + (long)tokens[r] * d;
    const float* p = pos + (long)(pos0 + (offset ? *offset : 0) + r % n_tok) * d;
    for (int c = threadIdx.x; c < d; c += 256) x[(long)r * d + c] = e[c] * scale + p[c];
}

// single-token steps replayed from a graph: tokens [rows] and the cache offset come from a host-coherent block (no copy
// node); workgroup 0 leaves the offset in device memory for the kernels behind it
__global__ __launch_bounds__(256) void nllb_embed_step_kernel(const int* __restrict__ host_block, int rows,
                                                              const float* __restrict__ emb, const float* __restrict__ pos,
                                                              float scale, int pos0, int d, int* __restrict__ offset_dev,
                                                              float* __restrict__ x) {
    const int r = blockIdx.x;
    const int tok = host_block[r], off = host_block[rows];
    if (r == 0 && threadIdx.x == 0) *offset_dev = off;
    const float* e = emb + (long)tok * d;
    const float* p = pos + (long)(pos0 + off) * d;
    for (int c = threadIdx.x; c < d; c += 256) x[(long)r * d + c] = e[c] * scale + p[c];
}

// AlignAtt read-out of one single-token step.  probs [n_align][rows][S] are the selected heads' softmax rows as
// decoder_cross_attention_kernel left them (rank-major).  One workgroup per row, S <= 512 = two positions per thread:
//   p[j]   = (probs[0][row][j] + probs[1][row][j] + ... in rank order) * (1 / n_align)
//   a      = the position of the largest p[j], j in [lo, hi), the lowest j on an exact tie; -1 when the window is empty
//   prob   = p[a] (0 when a = -1)
//   mass   = sum of p[j], j >= limit: per thread (j = tid) + (j = tid + 256), wave butterfly, then (w0 + w1) + (w2 + w3)
// lo / hi / limit are read from ctl[0..2] (a host-coherent block in a replayed step: the recording serves every window) and
// clamped to the row.  pos / prob / mass may be host-coherent too: one plain store each.
__global__ __launch_bounds__(256) void nllb_align_readout_kernel(const float* __restrict__ probs, int n_align, int rows, int S,
                                                                 float inv_n, const int* __restrict__ ctl,
                                                                 float* __restrict__ p_out, int* __restrict__ pos,
                                                                 float* __restrict__ prob, float* __restrict__ mass) {
    __shared__ float red_v[4], red_m[4];
    __shared__ int red_i[4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lo = max(ctl[0], 0), hi = min(ctl[1], S), limit = max(ctl[2], 0);
    const long head_stride = (long)rows * S;
    const float* base = probs + (long)row * S;
    float bv = -INFINITY, tail = 0.f;
    int bi = INT_MAX;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int j = tid + half * 256;
        if (j < S) {
            float acc = 0.f;
            for (int a = 0; a < n_align; ++a) acc += base[a * head_stride + j];
            const float p = acc * inv_n;
            p_out[(long)row * S + j] = p;
            if (j >= limit) tail += p;
            if (j >= lo && j < hi && p > bv) { bv = p; bi = j; }      // j ascends: an equal value keeps the lower position
        }
    }
    wave_argmax(bv, bi);
    tail = wave_sum(tail);
    if (lane == 0) { red_v[wave] = bv; red_i[wave] = bi; red_m[wave] = tail; }
    __syncthreads();
    if (tid == 0) {
        float v = red_v[0];
        int i = red_i[0];
        for (int w = 1; w < 4; ++w)
            if (red_v[w] > v || (red_v[w] == v && red_i[w] < i)) { v = red_v[w]; i = red_i[w]; }
        const bool found = i != INT_MAX;
        pos[row] = found ? i : -1;
        prob[row] = found ? v : 0.f;
        mass[row] = (red_m[0] + red_m[1]) + (red_m[2] + red_m[3]);
    }
}

void launch_nllb_align_readout(const LaunchCtx& ctx, const float* probs, int n_align, int rows, int S, const int* ctl,
                               float* p_out, int* pos, float* prob, float* mass) {
    if (n_align < 1 || n_align > kNlMaxAlign || rows < 1 || S < 1 || S > kSfMaxFrames)
        throw std::invalid_argument("NLLB alignment read-out: 1..64 heads, rows >= 1, 1..512 source positions");
    KernelScope ks(ctx, "nllb_align_readout");
    hipLaunchKernelGGL(nllb_align_readout_kernel, dim3(rows), dim3(256), 0, ctx.stream, probs, n_align, rows, S,
                       1.0f / (float)n_align, ctl, p_out, pos, prob, mass);
    WLK_HIP(hipGetLastError());
}

}  // namespace wlk

using namespace wlk;

struct wlk_nllb_session : NlOwner {
    // graphs[]: the plain, ancestry and align step, each per kv_cur; every one is re-recorded on another k / source length
    // (NlGraphSlot), the align pair also on another head set
    enum { kStepGraph = 0, kBeamGraph = 2, kAlignGraph = 4, kGraphs = 6 };
    wlk_nllb_session() : NlOwner(kGraphs) {}
    int rows = 1;
    // encoder
    float *ex = nullptr, *eh = nullptr, *eqkv = nullptr, *eatt = nullptr, *ewide = nullptr, *enc_out = nullptr, *cross_kv = nullptr;
    int src_len = 0;
    bool encoded = false;
    // decoder
    float *kcache[2] = {nullptr, nullptr}, *vcache[2] = {nullptr, nullptr};
    int kv_cur = 0;
    NlDecWs ws{};
    float *hsel = nullptr, *logits = nullptr;
    int *tokens_dev = nullptr, *offset_dev = nullptr, *src_rows_dev = nullptr;
    float* top_vals = nullptr;
    int* top_ids = nullptr;
    void* topk_scratch = nullptr;
    int self_len = 0;
    bool have_logits = false;
    // graph-replayed single-token steps (wlk_nllb_step)
    int* step_host = nullptr;          // pinned + mapped: [rows] tokens | offset ( | [rows] source rows | fresh: ancestry steps)
    int* step_host_dev = nullptr;      // the same block as the device sees it
    float* step_vals_host = nullptr;   // pinned + mapped: top-k results written by the top-k kernel itself
    int* step_ids_host = nullptr;
    float* step_vals_dev = nullptr;
    int* step_ids_dev = nullptr;
    // ancestry steps (wlk_nllb_step_beam): the step block continues [... | src rows | fresh]; no cache row moves
    unsigned char* anc = nullptr;      // [rows][max_tgt]: physical cache row that holds position t of hypothesis b
    void* topk_wide_scratch = nullptr;
    bool anc_live = false;             // an ancestry step has run since the last decode(first=1) / encode
    uint64_t ancestry_steps = 0;
    // AlignAtt steps (wlk_nllb_step_align): selected heads' softmax rows [n_align][rows][src_len] -> read-out
    int n_align = 0;
    int* head_rank_dev = nullptr;      // [dec_layers][heads]: rank of the (layer, head) pair or -1
    int* align_rows_dev = nullptr;     // [rows] zeros (ring row) | [rows] 0, 1, ... (beam of row)
    float* align_probs = nullptr;      // [kNlMaxAlign][rows][max_src]
    float* align_p = nullptr;          // [rows][max_src]: head mean of the latest align step
    int* align_host = nullptr;         // pinned + mapped: lo | hi | limit | [rows] position | [rows] probability | [rows] tail mass
    int* align_host_dev = nullptr;
    bool have_align = false;           // align_p holds a step of the current source
    uint64_t align_steps = 0, align_captures = 0;
};

namespace wlk {

// Session addressing of the decoder layers: the current dense caches [layer][row][ctx][d] at *offset_dev, one cross K/V and
// one source length for every row; anc / align as nl_decode's anc_step / align_step
struct NlSessionAddr {
    const wlk_nllb_session* s;
    int n_tok;
    bool anc, align;
    const wlk_nllb_dims& D() const { return s->m->D; }
    size_t cache_at(int l) const { return (size_t)l * s->rows * D().max_tgt * D().d_model; }
    float* kc(int l) const { return s->kcache[s->kv_cur] + cache_at(l); }
    float* vc(int l) const { return s->vcache[s->kv_cur] + cache_at(l); }
    void kv_rider(GemmArgs& g, int l) const {
        g.kcache = kc(l); g.vcache = vc(l); g.kv_pos = s->offset_dev; g.kv_d = D().d_model; g.kv_ctx = D().max_tgt;
    }
    void append(const LaunchCtx& c, const float* qkv, int l) const {
        launch_kv_append(c, qkv, kc(l), vc(l), s->rows, n_tok, s->offset_dev, D().d_model, D().max_tgt);
    }
    void self_attention(const LaunchCtx& c, const float* qkv, float* att, int l) const {
        if (anc) launch_decoder_self_attention_anc(c, qkv, kc(l), vc(l), s->anc, att, s->rows, s->offset_dev, D().d_model, D().heads, D().max_tgt);
        else launch_decoder_self_attention(c, qkv, kc(l), vc(l), att, s->rows, n_tok, s->offset_dev, D().d_model, D().heads, D().max_tgt);
    }
    void cross_attention(const LaunchCtx& c, const float* q, float* att, int l) const {
        const int d = D().d_model, H = D().heads, rows = s->rows;
        CrossAttnArgs ca{};
        ca.q = q;
        ca.k = s->cross_kv + (size_t)l * 2 * d;
        ca.v = ca.k + d;
        ca.ldkv = (long)D().dec_layers * 2 * d;
        ca.out = att;
        ca.rows = rows * n_tok; ca.d = d; ca.n_head = H; ca.T = s->src_len;
        ca.head_rank = nullptr; ca.ring = nullptr; ca.ring_row = nullptr; ca.beam_of_row = nullptr;
        ca.ring_rows = 0; ca.n_beam = 1; ca.qk_debug = nullptr;
        if (align) {          // window [n_align][rows][1][S]: row r is "beam" r, ring row 0
            ca.head_rank = s->head_rank_dev + (size_t)l * H;
            ca.ring = s->align_probs; ca.ring_row = s->align_rows_dev; ca.beam_of_row = s->align_rows_dev + rows;
            ca.ring_rows = 1; ca.n_beam = rows;
        }
        launch_decoder_cross_attention(c, ca);
    }
};

static void nl_encode(wlk_nllb_session* s, int S) {
    wlk_nllb* m = s->m;
    const wlk_nllb_dims& D = m->D;
    hipLaunchKernelGGL(nllb_embed_kernel, dim3(S), dim3(256), 0, s->stream, s->tokens_dev, m->emb, m->pos, D.embed_scale,
                       D.pad_id + 1, (const int*)nullptr, S, D.d_model, s->ex);
    WLK_HIP(hipGetLastError());
    SfAttnArgs one;
    one.T = S;
    nl_encoder_layers(s->ctx(), m, s->ex, s->eh, s->eqkv, s->eatt, s->ewide, s->enc_out, s->cross_kv, S, one);
}

// graph_k > 0: a single-token step replayed from a graph - tokens and offset come from the host-coherent step block and
// the graph_k best continuations of every row go straight back into host-coherent memory
// anc_step (n_tok == 1, graph replay): row b continues hypothesis src[b] of the previous step WITHOUT moving the cache - the
// table update runs in front of the layers and the self-attention reads keys / values through the table
// align_step (n_tok == 1, graph replay): the selected heads leave their softmax rows in align_probs and the read-out follows
// the top-k
static void nl_decode(wlk_nllb_session* s, int n_tok, int graph_k = 0, bool anc_step = false, bool align_step = false) {
    wlk_nllb* m = s->m;
    const wlk_nllb_dims& D = m->D;
    const LaunchCtx c = s->ctx();
    const int d = D.d_model, rows = s->rows, R = rows * n_tok;
    const bool graph_step = graph_k > 0, fused = n_tok == 1 && gemv_applicable(R, d);
    if (anc_step && (!fused || !graph_step || !s->anc)) throw std::logic_error("NLLB decode: the ancestry step needs the fused graph step");
    if (align_step && (n_tok != 1 || !graph_step || anc_step || s->n_align < 1))
        throw std::logic_error("NLLB decode: the alignment step is a single-token graph step with heads set");
    if (graph_step)
        hipLaunchKernelGGL(nllb_embed_step_kernel, dim3(R), dim3(256), 0, s->stream, s->step_host_dev, rows, m->emb, m->pos,
                           D.embed_scale, D.pad_id + 1, d, s->offset_dev, s->ws.x);
    else
        hipLaunchKernelGGL(nllb_embed_kernel, dim3(R), dim3(256), 0, s->stream, s->tokens_dev, m->emb, m->pos, D.embed_scale,
                           D.pad_id + 1, s->offset_dev, n_tok, d, s->ws.x);
    WLK_HIP(hipGetLastError());
    if (anc_step) launch_anc_update_block(c, s->anc, s->step_host_dev, rows, D.max_tgt);
    nl_decoder_layers(c, m, s->ws, R, fused, NlSessionAddr{s, n_tok, anc_step, align_step});
    nl_logits(c, m, fused, s->ws.x, rows, n_tok, s->hsel, s->logits);
    if (graph_k > 8)     // (ancestry steps only: wlk_nllb_step stops at 8)
        launch_logsoftmax_topk_wide(c, s->logits, D.vocab, rows, graph_k, s->step_vals_dev, s->step_ids_dev, s->topk_wide_scratch);
    else if (graph_step)      // results straight into the host-coherent block: no copy node behind the graph either
        launch_logsoftmax_topk(c, s->logits, D.vocab, rows, graph_k, s->step_vals_dev, s->step_ids_dev, s->topk_scratch, nullptr,
                               nullptr, nullptr, 0);
    if (align_step) {
        float* res = reinterpret_cast<float*>(s->align_host_dev + 3);
        launch_nllb_align_readout(c, s->align_probs, s->n_align, rows, s->src_len, s->align_host_dev, s->align_p, s->align_host_dev + 3,
                                  res + rows, res + 2 * rows);
    }
}

}  // namespace wlk

extern "C" {

int wlk_nllb_arena_floats(const wlk_nllb_dims* dims, uint64_t* n_floats) {
    if (int rc = nl_check_dims(dims)) return rc;
    if (!n_floats) return nl_fail(WLK_ERR_ARG, "NULL argument");
    nl_layout(*dims, n_floats);
    return WLK_OK;
}

int wlk_nllb_tensor_lookup(const wlk_nllb_dims* dims, const char* packed_name, uint64_t* offset_floats, uint64_t* numel) {
    if (int rc = nl_check_dims(dims)) return rc;
    if (!packed_name) return nl_fail(WLK_ERR_ARG, "NULL argument");
    for (const auto& s : nl_layout(*dims, nullptr))
        if (s.name == packed_name) {
            if (offset_floats) *offset_floats = s.offset;
            if (numel) *numel = s.numel;
            return WLK_OK;
        }
    return nl_fail(WLK_ERR_ARG, std::string("unknown packed tensor ") + packed_name);
}

int wlk_nllb_tensor_name(const wlk_nllb_dims* dims, int index, const char** name) {
    if (int rc = nl_check_dims(dims)) return rc;
    if (!name) return nl_fail(WLK_ERR_ARG, "NULL argument");
    static thread_local std::string hold;
    const auto v = nl_layout(*dims, nullptr);
    if (index < 0 || index >= (int)v.size()) return nl_fail(WLK_ERR_ARG, "tensor index out of range");
    hold = v[index].name;
    *name = hold.c_str();
    return WLK_OK;
}

int wlk_nllb_create(const wlk_nllb_dims* dims, int device, wlk_nllb** out) {
    if (int rc = nl_check_dims(dims)) return rc;
    if (!out) return nl_fail(WLK_ERR_ARG, "NULL argument");
    return nl_guarded([&]() {
        int n_dev = 0;
        if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)
            return nl_fail(WLK_ERR_HIP, "no HIP device: the NLLB backend has no CPU fallback");
        if (device < 0 || device >= n_dev) return nl_fail(WLK_ERR_ARG, "device index out of range");
        WLK_HIP(hipSetDevice(device));
        auto m = std::make_unique<wlk_nllb>();
        m->D = *dims;
        m->device = device;
        m->layout = nl_layout(*dims, &m->arena_floats);
        for (const auto& s : m->layout) m->index[s.name] = &s;
        WLK_HIP(hipMalloc(reinterpret_cast<void**>(&m->arena), m->arena_floats * sizeof(float)));
        memset_sync(m->arena, 0, m->arena_floats * sizeof(float));
        *out = m.release();
        return WLK_OK;
    });
}

int wlk_nllb_upload(wlk_nllb* m, const char* packed_name, const float* host, uint64_t numel) {
    if (!m || !packed_name || !host) return nl_fail(WLK_ERR_ARG, "NULL argument");
    return nl_guarded([&]() {
        auto it = m->index.find(packed_name);
        if (it == m->index.end()) return nl_fail(WLK_ERR_ARG, std::string("unknown packed tensor ") + packed_name);
        if (it->second->numel != numel)
            return nl_fail(WLK_ERR_ARG, std::string("size mismatch for ") + packed_name + ": expected " +
                                            std::to_string(it->second->numel) + ", got " + std::to_string(numel));
        WLK_HIP(hipSetDevice(m->device));
        copy_sync(m->arena + it->second->offset, host, numel * sizeof(float), hipMemcpyHostToDevice);
        m->finalized = false;
        return WLK_OK;
    });
}

int wlk_nllb_finalize(wlk_nllb* m) {
    if (!m) return nl_fail(WLK_ERR_ARG, "model is NULL");
    return nl_guarded([&]() {
        const wlk_nllb_dims& D = m->D;
        auto fill = [&](std::vector<NlLayer>& v, int n, const std::string& side, bool cross) {
            v.assign(n, NlLayer{});
            for (int i = 0; i < n; ++i) {
                const std::string p = side + "." + std::to_string(i) + ".";
                NlLayer& w = v[i];
                w.ln1w = m->P(p + "ln1.w"); w.ln1b = m->P(p + "ln1.b");
                w.qkvw = m->P(p + "qkv.w"); w.qkvb = m->P(p + "qkv.b");
                w.outw = m->P(p + "out.w"); w.outb = m->P(p + "out.b");
                if (cross) {
                    w.lnxw = m->P(p + "lnx.w"); w.lnxb = m->P(p + "lnx.b");
                    w.xqw = m->P(p + "xq.w"); w.xqb = m->P(p + "xq.b");
                    w.xkvw = m->P(p + "xkv.w"); w.xkvb = m->P(p + "xkv.b");
                    w.xoutw = m->P(p + "xout.w"); w.xoutb = m->P(p + "xout.b");
                }
                w.ln2w = m->P(p + "ln2.w"); w.ln2b = m->P(p + "ln2.b");
                w.fc1w = m->P(p + "fc1.w"); w.fc1b = m->P(p + "fc1.b");
                w.fc2w = m->P(p + "fc2.w"); w.fc2b = m->P(p + "fc2.b");
            }
        };
        fill(m->enc, D.enc_layers, "enc", false);
        fill(m->dec, D.dec_layers, "dec", true);
        m->emb = m->P("shared.emb"); m->pos = m->P("pos.table");
        m->enc_lnw = m->P("enc.ln.w"); m->enc_lnb = m->P("enc.ln.b");
        m->dec_lnw = m->P("dec.ln.w"); m->dec_lnb = m->P("dec.ln.b");
        m->finalized = true;
        return WLK_OK;
    });
}

int wlk_nllb_destroy(wlk_nllb* m) {
    delete m;        // sessions and batches (nllb_batch.hip) of the model must be destroyed first (they hold pointers into its arena)
    return WLK_OK;
}

int wlk_nllb_session_create(wlk_nllb* m, int rows, wlk_nllb_session** out) {
    if (!m || !out) return nl_fail(WLK_ERR_ARG, "NULL argument");
    if (!m->finalized) return nl_fail(WLK_ERR_STATE, "NLLB model not finalized");
    if (rows < 1 || rows > 8) return nl_fail(WLK_ERR_ARG, "NLLB session: 1..8 hypothesis rows");
    return nl_guarded([&]() {
        WLK_HIP(hipSetDevice(m->device));
        auto s = std::make_unique<wlk_nllb_session>();
        s->m = m;
        s->rows = rows;
        WLK_HIP(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
        const wlk_nllb_dims& D = m->D;
        const size_t d = D.d_model, f = D.ffn, S = D.max_src, Tt = D.max_tgt, Rmax = (size_t)rows * Tt;
        s->ex = s->alloc<float>(S * d); s->eh = s->alloc<float>(S * d); s->eqkv = s->alloc<float>(S * 3 * d);
        s->eatt = s->alloc<float>(S * d); s->ewide = s->alloc<float>(S * f); s->enc_out = s->alloc<float>(S * d);
        s->cross_kv = s->alloc<float>(S * D.dec_layers * 2 * d);
        for (int i = 0; i < 2; ++i) {
            s->kcache[i] = s->alloc<float>((size_t)D.dec_layers * rows * Tt * d);
            s->vcache[i] = s->alloc<float>((size_t)D.dec_layers * rows * Tt * d);
        }
        s->ws = NlDecWs{s->alloc<float>(Rmax * d), s->alloc<float>(Rmax * d), s->alloc<float>(Rmax * 3 * d), s->alloc<float>(Rmax * d),
                        s->alloc<float>(Rmax * d), s->alloc<float>(Rmax * f)};
        s->hsel = s->alloc<float>((size_t)rows * d);
        s->logits = s->alloc<float>((size_t)rows * D.vocab);
        s->tokens_dev = s->alloc<int>(std::max(S, Rmax));
        s->offset_dev = s->alloc<int>(1);
        s->src_rows_dev = s->alloc<int>(rows);
        s->top_vals = s->alloc<float>((size_t)rows * 16);
        s->top_ids = s->alloc<int>((size_t)rows * 16);
        s->topk_scratch = s->alloc<char>(topk_scratch_bytes(rows));
        s->topk_wide_scratch = s->alloc<char>(topk_wide_scratch_bytes(rows));
        s->anc = s->alloc<unsigned char>((size_t)rows * Tt);
        WLK_HIP(hipMemsetAsync(s->anc, 0, (size_t)rows * Tt, s->stream));
        WLK_HIP(hipStreamSynchronize(s->stream));
        // [tokens rows | offset] for wlk_nllb_step, continued by [src rows | fresh] for wlk_nllb_step_beam
        s->mapped((size_t)(2 * rows + 2), &s->step_host, &s->step_host_dev);
        s->mapped((size_t)rows * 16, &s->step_vals_host, &s->step_vals_dev);
        s->mapped((size_t)rows * 16, &s->step_ids_host, &s->step_ids_dev);
        *out = s.release();
        return WLK_OK;
    });
}

int wlk_nllb_session_destroy(wlk_nllb_session* s) {
    delete s;        // ~wlk_nllb_session releases the stream, graphs and buffers
    return WLK_OK;
}

static int nl_stage_tokens(wlk_nllb_session* s, const int64_t* ids, int n, std::vector<int>& stage) {
    const wlk_nllb_dims& D = s->m->D;
    if (int rc = nl_check_tokens(D, ids, n, "padding inside a sequence is not supported (one sentence per call)")) return rc;
    stage.assign(ids, ids + n);
    return WLK_OK;
}

int wlk_nllb_encode(wlk_nllb_session* s, const int64_t* src_ids, int32_t n) {
    if (!s || !src_ids) return nl_fail(WLK_ERR_ARG, "NULL argument");
    if (n < 1 || n > s->m->D.max_src) return nl_fail(WLK_ERR_CAPACITY, "source length out of range");
    return nl_guarded([&]() {
        std::vector<int> stage;
        if (int rc = nl_stage_tokens(s, src_ids, n, stage)) return rc;
        WLK_HIP(hipSetDevice(s->m->device));
        WLK_HIP(hipStreamSynchronize(s->stream));
        WLK_HIP(hipMemcpyAsync(s->tokens_dev, stage.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, s->stream));
        WLK_HIP(hipStreamSynchronize(s->stream));
        s->src_len = n;
        nl_encode(s, n);
        s->encoded = true;
        s->self_len = 0;
        s->have_logits = false;
        s->anc_live = false;
        s->have_align = false;
        return WLK_OK;
    });
}

int wlk_nllb_decode(wlk_nllb_session* s, const int64_t* tokens, int32_t n_rows, int32_t n_tok, int32_t first) {
    if (!s || !tokens) return nl_fail(WLK_ERR_ARG, "NULL argument");
    if (!s->encoded) return nl_fail(WLK_ERR_STATE, "wlk_nllb_decode before wlk_nllb_encode");
    if (n_rows != s->rows) return nl_fail(WLK_ERR_ARG, "n_rows must equal the session's row count");
    if (n_tok < 1) return nl_fail(WLK_ERR_ARG, "n_tok must be >= 1");
    if (!first && s->anc_live)
        return nl_fail(WLK_ERR_STATE, "wlk_nllb_decode(first=0) after an ancestry step: the cache rows are no longer the hypotheses");
    return nl_guarded([&]() {
        if (first) s->self_len = 0;
        else if (s->self_len == 0) return nl_fail(WLK_ERR_STATE, "the first decode after an encode must set first=1");
        if (s->self_len + n_tok > s->m->D.max_tgt) return nl_fail(WLK_ERR_CAPACITY, "target context exceeded");
        std::vector<int> stage;
        if (int rc = nl_stage_tokens(s, tokens, n_rows * n_tok, stage)) return rc;
        stage.push_back(s->self_len);
        WLK_HIP(hipSetDevice(s->m->device));
        WLK_HIP(hipStreamSynchronize(s->stream));
        WLK_HIP(hipMemcpyAsync(s->tokens_dev, stage.data(), (size_t)n_rows * n_tok * sizeof(int), hipMemcpyHostToDevice, s->stream));
        WLK_HIP(hipMemcpyAsync(s->offset_dev, stage.data() + (size_t)n_rows * n_tok, sizeof(int), hipMemcpyHostToDevice, s->stream));
        WLK_HIP(hipStreamSynchronize(s->stream));           // `stage` is pageable
        nl_decode(s, n_tok);
        s->self_len += n_tok;
        s->have_logits = true;
        if (first) s->anc_live = false;
        return WLK_OK;
    });
}

int wlk_nllb_step(wlk_nllb_session* s, const int64_t* tokens, int32_t n_rows, int32_t k, float* logprobs, int32_t* ids) {
    if (!s || !tokens || !logprobs || !ids) return nl_fail(WLK_ERR_ARG, "NULL argument");
    if (!s->encoded || s->self_len == 0) return nl_fail(WLK_ERR_STATE, "wlk_nllb_step before the decoder prompt (wlk_nllb_decode first=1)");
    if (s->anc_live) return nl_fail(WLK_ERR_STATE, "wlk_nllb_step after an ancestry step: the cache rows are no longer the hypotheses");
    if (n_rows != s->rows) return nl_fail(WLK_ERR_ARG, "n_rows must equal the session's row count");
    if (k < 1 || k > 8) return nl_fail(WLK_ERR_ARG, "k must be 1..8 (the top-k kernel's limit)");
    const wlk_nllb_dims& D = s->m->D;
    if (s->self_len + 1 > D.max_tgt) return nl_fail(WLK_ERR_CAPACITY, "target context exceeded");
    if (!gemv_applicable(n_rows, D.d_model)) return nl_fail(WLK_ERR_ARG, "wlk_nllb_step: too many rows for the single-token path");
    if (int rc = nl_check_tokens(D, tokens, n_rows)) return rc;
    return nl_guarded([&]() {
        WLK_HIP(hipSetDevice(s->m->device));
        WLK_HIP(hipStreamSynchronize(s->stream));           // the previous step's readers of the host block are done
        for (int r = 0; r < n_rows; ++r) s->step_host[r] = (int)tokens[r];
        s->step_host[n_rows] = s->self_len;
        nl_replay(s->stream, s->graphs[s->kStepGraph + s->kv_cur], k, s->src_len, [&] { nl_decode(s, 1, k); });
        std::memcpy(logprobs, s->step_vals_host, (size_t)n_rows * k * sizeof(float));
        std::memcpy(ids, s->step_ids_host, (size_t)n_rows * k * sizeof(int));
        s->self_len += 1;
        s->have_logits = true;
        return WLK_OK;
    });
}

int wlk_nllb_step_beam(wlk_nllb_session* s, const int64_t* tokens, const int32_t* source_rows, int32_t n_rows, int32_t k,
                       float* logprobs, int32_t* ids) {
    if (!s || !tokens || !source_rows || !logprobs || !ids) return nl_fail(WLK_ERR_ARG, "NULL argument");
    if (!s->encoded || s->self_len == 0) return nl_fail(WLK_ERR_STATE, "wlk_nllb_step_beam before the decoder prompt (wlk_nllb_decode first=1)");
    if (n_rows != s->rows) return nl_fail(WLK_ERR_ARG, "n_rows must equal the session's row count");
    if (k < 1 || k > kTopkWideMaxK) return nl_fail(WLK_ERR_ARG, "k must be 1..16 (the wide top-k kernel's limit)");
    const wlk_nllb_dims& D = s->m->D;
    if (D.max_tgt > 512) return nl_fail(WLK_ERR_ARG, "wlk_nllb_step_beam: max_tgt must be <= 512 (the ancestry attention's limit)");
    if (!gemv_applicable(n_rows, D.d_model)) return nl_fail(WLK_ERR_ARG, "wlk_nllb_step_beam: too many rows for the single-token path");
    if (k > 8 && !topk_wide_applicable(D.vocab, k)) return nl_fail(WLK_ERR_ARG, "wlk_nllb_step_beam: k > 8 needs a vocabulary of at most 262144");
    if (s->self_len + 1 > D.max_tgt) return nl_fail(WLK_ERR_CAPACITY, "target context exceeded");
    for (int r = 0; r < n_rows; ++r) {
        if (int rc = nl_check_tokens(D, tokens + r, 1)) return rc;
        if (source_rows[r] < 0 || source_rows[r] >= n_rows) return nl_fail(WLK_ERR_ARG, "source row out of range");
    }
    return nl_guarded([&]() {
        WLK_HIP(hipSetDevice(s->m->device));
        WLK_HIP(hipStreamSynchronize(s->stream));           // the previous step's readers of the host block are done
        for (int r = 0; r < n_rows; ++r) {
            s->step_host[r] = (int)tokens[r];
            s->step_host[n_rows + 1 + r] = source_rows[r];
        }
        s->step_host[n_rows] = s->self_len;
        s->step_host[2 * n_rows + 1] = s->anc_live ? 0 : 1;      // fresh: every physical row still holds its own history
        nl_replay(s->stream, s->graphs[s->kBeamGraph + s->kv_cur], k, s->src_len,
                  [&] { nl_decode(s, 1, k, /*anc_step=*/true); });
        std::memcpy(logprobs, s->step_vals_host, (size_t)n_rows * k * sizeof(float));
        std::memcpy(ids, s->step_ids_host, (size_t)n_rows * k * sizeof(int));
        s->self_len += 1;
        s->have_logits = true;
        s->anc_live = true;
        s->ancestry_steps += 1;
        return WLK_OK;
    });
}

int wlk_nllb_session_beam_stats(wlk_nllb_session* s, uint64_t* ancestry_steps) {
    if (!s || !ancestry_steps) return nl_fail(WLK_ERR_ARG, "NULL argument");
    *ancestry_steps = s->ancestry_steps;
    return WLK_OK;
}

int wlk_nllb_session_set_align(wlk_nllb_session* s, const int32_t* layer_head_pairs, int32_t n) {
    if (!s || (n > 0 && !layer_head_pairs)) return nl_fail(WLK_ERR_ARG, "NULL argument");
    if (n < 0 || n > kNlMaxAlign) return nl_fail(WLK_ERR_ARG, "wlk_nllb_session_set_align: 0..64 (layer, head) pairs");
    const wlk_nllb_dims& D = s->m->D;
    std::vector<int> rank;
    if (int rc = nl_head_rank(D, layer_head_pairs, n, rank)) return rc;
    return nl_guarded([&]() {
        WLK_HIP(hipSetDevice(s->m->device));
        WLK_HIP(hipStreamSynchronize(s->stream));
        for (int i = 0; i < 2; ++i) s->graphs[s->kAlignGraph + i].drop();        // a recording carries the head count by value
        s->have_align = false;
        s->n_align = 0;
        if (n == 0) return WLK_OK;
        const int rows = s->rows;
        if (!s->align_host) {
            s->head_rank_dev = s->alloc<int>(rank.size());
            s->align_rows_dev = s->alloc<int>(2 * (size_t)rows);
            s->align_probs = s->alloc<float>((size_t)kNlMaxAlign * rows * D.max_src);
            s->align_p = s->alloc<float>((size_t)rows * D.max_src);
            s->mapped((size_t)(3 + 3 * rows), &s->align_host, &s->align_host_dev);
            std::vector<int> rr(2 * (size_t)rows, 0);
            for (int r = 0; r < rows; ++r) rr[rows + r] = r;
            copy_sync(s->align_rows_dev, rr.data(), rr.size() * sizeof(int), hipMemcpyHostToDevice);
        }
        copy_sync(s->head_rank_dev, rank.data(), rank.size() * sizeof(int), hipMemcpyHostToDevice);
        s->n_align = n;
        return WLK_OK;
    });
}

// the checks of wlk_nllb_step_align and one replay of the align graph; results stay in the host-coherent blocks
static int nl_step_align(wlk_nllb_session* s, const int64_t* tokens, int n_rows, int k, int lo, int hi, int limit) {
    if (!s->encoded || s->self_len == 0) return nl_fail(WLK_ERR_STATE, "wlk_nllb_step_align before the decoder prompt (wlk_nllb_decode first=1)");
    if (s->n_align < 1) return nl_fail(WLK_ERR_STATE, "wlk_nllb_step_align before wlk_nllb_session_set_align");
    if (s->anc_live) return nl_fail(WLK_ERR_STATE, "wlk_nllb_step_align after an ancestry step: the cache rows are no longer the hypotheses");
    if (n_rows != s->rows) return nl_fail(WLK_ERR_ARG, "n_rows must equal the session's row count");
    if (k < 1 || k > 8) return nl_fail(WLK_ERR_ARG, "k must be 1..8 (the top-k kernel's limit)");
    if (lo < 0 || hi > s->src_len || limit < 0 || limit > s->src_len)
        return nl_fail(WLK_ERR_ARG, "wlk_nllb_step_align: needs 0 <= lo, hi <= src_len and 0 <= limit <= src_len");
    const wlk_nllb_dims& D = s->m->D;
    if (s->self_len + 1 > D.max_tgt) return nl_fail(WLK_ERR_CAPACITY, "target context exceeded");
    if (!gemv_applicable(n_rows, D.d_model)) return nl_fail(WLK_ERR_ARG, "wlk_nllb_step_align: too many rows for the single-token path");
    if (int rc = nl_check_tokens(D, tokens, n_rows)) return rc;
    return nl_guarded([&]() {
        WLK_HIP(hipSetDevice(s->m->device));
        WLK_HIP(hipStreamSynchronize(s->stream));           // the previous step's readers of the host blocks are done
        for (int r = 0; r < n_rows; ++r) s->step_host[r] = (int)tokens[r];
        s->step_host[n_rows] = s->self_len;
        s->align_host[0] = lo; s->align_host[1] = hi; s->align_host[2] = limit;
        if (nl_replay(s->stream, s->graphs[s->kAlignGraph + s->kv_cur], k, s->src_len,
                      [&] { nl_decode(s, 1, k, /*anc_step=*/false, /*align_step=*/true); }))
            s->align_captures += 1;
        s->self_len += 1;
        s->have_logits = true;
        s->have_align = true;
        s->align_steps += 1;
        return WLK_OK;
    });
}

int wlk_nllb_step_align(wlk_nllb_session* s, const int64_t* tokens, int32_t n_rows, int32_t k, int32_t lo, int32_t hi, int32_t limit,
                        float* logprobs, int32_t* ids, int32_t* align_pos, float* align_prob, float* tail_mass) {
    if (!s || !tokens || !logprobs || !ids || !align_pos || !align_prob || !tail_mass) return nl_fail(WLK_ERR_ARG, "NULL argument");
    if (int rc = nl_step_align(s, tokens, n_rows, k, lo, hi, limit)) return rc;
    std::memcpy(logprobs, s->step_vals_host, (size_t)n_rows * k * sizeof(float));
    std::memcpy(ids, s->step_ids_host, (size_t)n_rows * k * sizeof(int));
    std::memcpy(align_pos, s->align_host + 3, (size_t)n_rows * sizeof(int));
    std::memcpy(align_prob, s->align_host + 3 + n_rows, (size_t)n_rows * sizeof(float));
    std::memcpy(tail_mass, s->align_host + 3 + 2 * n_rows, (size_t)n_rows * sizeof(float));
    return WLK_OK;
}

/* The AlignAtt rule (restated in whisperlivekit_amd.nllb.generate_alignatt for device_loop=False). */
int wlk_nllb_generate_alignatt(wlk_nllb_session* s, const int64_t* prompt, int32_t n_prompt, int32_t n_accessible, int32_t threshold,
                               int32_t final, int64_t eos_id, int32_t max_new, int64_t* out_ids, int32_t* out_align, int32_t* n_out,
                               int32_t* stop_reason) {
    if (!s || !prompt || !n_out || !stop_reason || (max_new > 0 && (!out_ids || !out_align))) return nl_fail(WLK_ERR_ARG, "NULL argument");
    if (s->rows != 1) return nl_fail(WLK_ERR_ARG, "wlk_nllb_generate_alignatt: needs a 1-row session");
    if (n_prompt < 2) return nl_fail(WLK_ERR_ARG, "wlk_nllb_generate_alignatt: the prompt needs at least two tokens (</s>, target language)");
    if (max_new < 0 || threshold < 0) return nl_fail(WLK_ERR_ARG, "wlk_nllb_generate_alignatt: max_new and threshold must be >= 0");
    if (!s->encoded) return nl_fail(WLK_ERR_STATE, "wlk_nllb_generate_alignatt before wlk_nllb_encode");
    if (s->n_align < 1) return nl_fail(WLK_ERR_STATE, "wlk_nllb_generate_alignatt before wlk_nllb_session_set_align");
    const int S = s->src_len;
    if (n_accessible < 0 || n_accessible > S) return nl_fail(WLK_ERR_ARG, "wlk_nllb_generate_alignatt: n_accessible must be 0..src_len");
    const int lo = 1, hi = S - 1;                    // the content between the language code and </s>
    const int limit = std::min(std::max(n_accessible - threshold, lo), S);
    *n_out = 0;
    if (int rc = wlk_nllb_decode(s, prompt, 1, n_prompt - 1, 1)) return rc;
    int64_t last = prompt[n_prompt - 1];
    int n = 0;
    for (;;) {
        if (n >= max_new) { *stop_reason = WLK_ALIGN_STOP_LENGTH; break; }
        if (s->self_len + 1 > s->m->D.max_tgt) { *stop_reason = WLK_ALIGN_STOP_CONTEXT; break; }
        if (int rc = nl_step_align(s, &last, 1, 1, lo, hi, limit)) return rc;
        const int64_t y = s->step_ids_host[0];
        const int a = s->align_host[3];
        if (!final && (a < 0 || a >= limit)) { *stop_reason = WLK_ALIGN_STOP_ATTENTION; break; }
        if (y == eos_id) { *stop_reason = WLK_ALIGN_STOP_EOS; break; }
        out_ids[n] = y;
        out_align[n] = a;
        last = y;
        *n_out = ++n;
    }
    return WLK_OK;
}

int wlk_nllb_session_align_stats(wlk_nllb_session* s, uint64_t* align_steps, uint64_t* graph_captures) {
    if (!s || !align_steps || !graph_captures) return nl_fail(WLK_ERR_ARG, "NULL argument");
    *align_steps = s->align_steps;
    *graph_captures = s->align_captures;
    return WLK_OK;
}

int wlk_nllb_kv_reorder(wlk_nllb_session* s, const int32_t* source_rows, int32_t n_rows) {
    if (!s || !source_rows) return nl_fail(WLK_ERR_ARG, "NULL argument");
    if (n_rows != s->rows) return nl_fail(WLK_ERR_ARG, "n_rows must equal the session's row count");
    if (s->anc_live) return nl_fail(WLK_ERR_STATE, "wlk_nllb_kv_reorder after an ancestry step: the cache rows are no longer the hypotheses");
    bool identity = true;
    for (int i = 0; i < n_rows; ++i) {
        if (source_rows[i] < 0 || source_rows[i] >= n_rows) return nl_fail(WLK_ERR_ARG, "source row out of range");
        identity = identity && source_rows[i] == i;
    }
    if (identity || s->self_len == 0) return WLK_OK;
    return nl_guarded([&]() {
        const wlk_nllb_dims& D = s->m->D;
        WLK_HIP(hipSetDevice(s->m->device));
        WLK_HIP(hipStreamSynchronize(s->stream));
        WLK_HIP(hipMemcpyAsync(s->src_rows_dev, source_rows, (size_t)n_rows * sizeof(int), hipMemcpyHostToDevice, s->stream));
        WLK_HIP(hipStreamSynchronize(s->stream));
        const LaunchCtx c = s->ctx();
        const int nxt = s->kv_cur ^ 1;
        launch_kv_gather(c, s->kcache[s->kv_cur], s->kcache[nxt], s->src_rows_dev, n_rows, s->self_len, D.d_model, D.max_tgt, D.dec_layers);
        launch_kv_gather(c, s->vcache[s->kv_cur], s->vcache[nxt], s->src_rows_dev, n_rows, s->self_len, D.d_model, D.max_tgt, D.dec_layers);
        s->kv_cur = nxt;
        return WLK_OK;
    });
}

int wlk_nllb_topk(wlk_nllb_session* s, int32_t k, float* logprobs, int32_t* ids) {
    if (!s || !logprobs || !ids) return nl_fail(WLK_ERR_ARG, "NULL argument");
    if (!s->have_logits) return nl_fail(WLK_ERR_STATE, "wlk_nllb_topk before a decode");
    if (k < 1 || k > kTopkWideMaxK) return nl_fail(WLK_ERR_ARG, "k must be 1..16 (the wide top-k kernel's limit)");
    return nl_guarded([&]() {
        WLK_HIP(hipSetDevice(s->m->device));
        if (k > 8)
            launch_logsoftmax_topk_wide(s->ctx(), s->logits, s->m->D.vocab, s->rows, k, s->top_vals, s->top_ids, s->topk_wide_scratch);
        else
            launch_logsoftmax_topk(s->ctx(), s->logits, s->m->D.vocab, s->rows, k, s->top_vals, s->top_ids, s->topk_scratch, nullptr,
                                   nullptr, nullptr, 0);
        WLK_HIP(hipMemcpyAsync(logprobs, s->top_vals, (size_t)s->rows * k * sizeof(float), hipMemcpyDeviceToHost, s->stream));
        WLK_HIP(hipMemcpyAsync(ids, s->top_ids, (size_t)s->rows * k * sizeof(int), hipMemcpyDeviceToHost, s->stream));
        WLK_HIP(hipStreamSynchronize(s->stream));
        return WLK_OK;
    });
}

int wlk_nllb_export(wlk_nllb_session* s, const char* what, float* host, uint64_t capacity, uint64_t* n_written) {
    if (!s || !what || !host || !n_written) return nl_fail(WLK_ERR_ARG, "NULL argument");
    return nl_guarded([&]() {
        const wlk_nllb_dims& D = s->m->D;
        const std::string w = what;
        const float* src = nullptr;
        uint64_t n = 0;
        if (w == "logits") {
            if (!s->have_logits) return nl_fail(WLK_ERR_STATE, "no logits yet");
            src = s->logits; n = (uint64_t)s->rows * D.vocab;
        } else if (w == "enc") {
            if (!s->encoded) return nl_fail(WLK_ERR_STATE, "not encoded");
            src = s->enc_out; n = (uint64_t)s->src_len * D.d_model;
        } else if (w == "align") {
            if (!s->have_align) return nl_fail(WLK_ERR_STATE, "no alignment step yet");
            src = s->align_p; n = (uint64_t)s->rows * s->src_len;
        } else {
            return nl_fail(WLK_ERR_ARG, "unknown export " + w);
        }
        if (n > capacity) return nl_fail(WLK_ERR_CAPACITY, "export buffer too small");
        WLK_HIP(hipSetDevice(s->m->device));
        WLK_HIP(hipMemcpyAsync(host, src, n * sizeof(float), hipMemcpyDeviceToHost, s->stream));
        WLK_HIP(hipStreamSynchronize(s->stream));
        *n_written = n;
        return WLK_OK;
    });
}

int wlk_nllb_sync(wlk_nllb_session* s) {
    if (!s) return nl_fail(WLK_ERR_ARG, "NULL argument");
    return nl_guarded([&]() {
        WLK_HIP(hipSetDevice(s->m->device));
        WLK_HIP(hipStreamSynchronize(s->stream));
        return WLK_OK;
    });
}

}  // extern "C"
