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
// wlk_group_run_pick takes up to 16 such steps behind one call: everything the next step needs from the host - the
// next StepRow, the next rule state, whether the row goes on - is a pure function of the previous pick, so a one-wave kernel
// (group_advance_rows_kernel) derives it on the device between two chains.  The host enqueues `burst` chains back to back,
// reads the picks and the per-row step counts back once and synchronises once.  wlk_group_step_pick is its one-step case.
//
// The layer chain is the batch engine's, wlk_enqueue_step_rows (decoder_chain.hip), without the one-row fold of the
// cross-attention's query projection: a row goes through the same kernels whether it steps alone or beside seven others.
//
// The same group also aligns the words of up to 8 windows in one call (wlk_group_find_alignment): one stacked
// teacher-forced decoder pass (decoder_chain.hip: wlk_prefill_chain), the token probabilities per window, the ragged normalisation
// (word_align.hip), the warping recurrences side by side and the path walk on the device (dtw.hip), one read-back of the
// starts and probabilities.  Its workspace is allocated by the first such call.
//
// And it verifies drafts (wlk_group_verify): the same stacked pass over [initial tokens | draft] of up to 8
// windows, the greedy pick of every candidate position with the rule state its history gives, the accepted prefix and the
// token behind it on the device (select.hip: draft_pick_rows_kernel, draft_accept_kernel), 32 bytes back per window; each
// session is left as its own prefill of the accepted tokens leaves it.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "common.h"
#include "decoder_chain.h"
#include "internal.h"

using namespace wlk;

namespace {
constexpr int kGroupMaxRows = 8;
constexpr int kGroupMaxBurst = 16;
// a row's state across the chains of one call (wlk_group_run_pick), advanced on the device
struct BurstRow {
    int alive;                             // the row takes the next chain as a step of its own
    int taken;                             // own steps so far in this call
    int limit;                             // own steps at most: min(max_steps, burst, free text positions)
    int n_steps, self_len, prefill_rows;   // the session's counters before the row's next own step (step_row_scalars)
};
// what one call uploads, in one copy: the row table the layer kernels index, the rule table of the pick and - for a call of
// more than one chain - the burst records
struct GroupBlock {
    StepRow rows[kGroupMaxRows];
    PickRowEntry pick[kGroupMaxRows];
    BurstRow burst[kGroupMaxRows];
};
// what a call of more than one chain reads back, in one copy
struct GroupResults {
    int picks[kGroupMaxRows][kGroupMaxBurst][2];   // [row][own step][token | log-probability bits]
    int taken[kGroupMaxRows];                      // own steps of every row
};
// a device block that grows on demand and is freed with its owner
struct GrowBuf {
    char* p = nullptr;
    size_t cap = 0;
    GrowBuf() = default;
    GrowBuf(const GrowBuf&) = delete;
    ~GrowBuf() { if (p) (void)hipFree(p); }
    void reserve(size_t bytes, hipStream_t stream) {
        if (bytes <= cap) return;
        WLK_HIP(hipStreamSynchronize(stream));     // what the stream still has queued reads the old block
        if (p) WLK_HIP(hipFree(p));
        p = nullptr; cap = 0;
        p = dev_alloc<char>(bytes);
        cap = bytes;
    }
};

// Between two chains of a call: one wave, lane r = row r.  A live row's pick goes to its next result slot; unless that pick
// was <|endoftext|> or the row's last allowed step, its StepRow and rule state become those of its next step.
// A row that has ended is left untouched, and so is its table entry: in the remaining chains of the call it REPEATS its last
// step - the same token at the same offset, into the same cache slot and the same alignment-window row.  Every kernel of
// the chain is a deterministic function of its row's inputs, and a step reads the cache positions below its offset and
// writes the one at it, so the repeat rewrites the values that are already there (the argument of the padded tile rows of
// wlk_prefill_group).  A dead row therefore needs no guard in any layer kernel, its logits row
// (wlk_group_export_logits) and its pick slot keep showing its last own step, and nothing its session owns differs from
// what `taken` single steps leave.
__global__ __launch_bounds__(64) void group_advance_rows_kernel(GroupBlock* __restrict__ blk, const int* __restrict__ pick,
                                                                 GroupResults* __restrict__ res, int n, int n_text_ctx) {
    const int r = threadIdx.x;
    if (r >= n || r >= kGroupMaxRows) return;
    BurstRow b = blk->burst[r];
    if (!b.alive || b.taken < 0 || b.taken >= kGroupMaxBurst) return;
    const int token = pick[2 * r];
    res->picks[r][b.taken][0] = token;
    res->picks[r][b.taken][1] = pick[2 * r + 1];
    b.taken += 1;
    res->taken[r] = b.taken;
    const PickRules p = blk->pick[r].p;
    if (token == p.eot || b.taken >= b.limit) {
        b.alive = 0;
    } else {
        b.n_steps += 1;
        b.self_len += 1;
        StepRow row = blk->rows[r];
        step_row_scalars(row, b.n_steps, b.self_len, b.prefill_rows, n_text_ctx, token, row.content_len);
        blk->rows[r] = row;
        blk->pick[r].p = pick_rules_advance(p, token);
    }
    blk->burst[r] = b;
}

// wlk_diag_pick_advance: pick_rules_advance alone
__global__ __launch_bounds__(256) void pick_advance_kernel(const PickRules* __restrict__ in, const int* __restrict__ tokens, int n,
                                                            PickRules* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = pick_rules_advance(in[i], tokens[i]);
}
}  // namespace

struct wlk_group {
    wlk_model* m = nullptr;
    int max_rows = 1;
    hipStream_t stream = nullptr;
    wlk_step_ws ws;                      // the activations of the step chain
    GroupBlock* blk_dev = nullptr;
    int* pick_dev = nullptr;             // [R][token | log-probability]
    GroupResults* results_dev = nullptr; // a call of more than one chain: every row's picks and step count
    char* pinned = nullptr;              // [GroupBlock | GroupResults (a one-chain call: R x 8 bytes of it)]
    hipEvent_t joined[kGroupMaxRows] = {};
    int last_rows = 0;                   // rows of the last completed step (wlk_group_export_logits)
    uint64_t n_steps = 0, n_rows = 0;
    std::mutex mu;                       // one step at a time
    // stacked word alignment (wlk_group_find_alignment): nothing of it exists before the first such call
    wlk_prefill_ws align_ws;             // the stacked decoder pass over 8 x 256 rows
    bool align_ready = false;
    GrowBuf align_buf;                   // [hidden | logits | w | cost | results | trace_t | trace]
    char* align_up_dev = nullptr;        // [AlignWin x 8 | targets int x 8 x 256]
    char* align_pinned = nullptr;        // [upload block | results: starts and token probabilities of all windows]
    // draft verification (wlk_group_verify): shares the stacked decoder pass's workspace; nothing of it exists before the
    // first such call
    GrowBuf verify_buf;                  // [hidden (n_d + 2) x d | logits (n_d + 2) x V] of the longest draft
    int* verify_dev = nullptr;           // [drafts int x 8 x 256 | picks int x 8 x 257 x 3 | results int x 8 x 8]
    int* verify_pinned = nullptr;        // [drafts | results]

    ~wlk_group() {
        (void)hipSetDevice(m->device);
        if (stream) (void)hipStreamSynchronize(stream);
        wlk_step_ws_free(ws);
        if (blk_dev) (void)hipFree(blk_dev);
        if (pick_dev) (void)hipFree(pick_dev);
        if (results_dev) (void)hipFree(results_dev);
        if (pinned) (void)hipHostFree(pinned);
        if (align_ready) wlk_prefill_ws_free(align_ws);
        if (align_up_dev) (void)hipFree(align_up_dev);
        if (align_pinned) (void)hipHostFree(align_pinned);
        if (verify_dev) (void)hipFree(verify_dev);
        if (verify_pinned) (void)hipHostFree(verify_pinned);
        for (hipEvent_t e : joined)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }

    // embed .. logits of R rows + every row's pick
    void enqueue_step(int R) {
        const LaunchCtx c{stream, nullptr};
        wlk_enqueue_step_rows(m, c, ws, blk_dev->rows, R);
        launch_rules_pick_rows(c, ws.logits, m->D.n_vocab, R, blk_dev->pick, pick_dev);
    }
    // what session s's own stream has queued (encode, prefill, its earlier steps) is done before this stream touches its caches
    void join(int r, const wlk_session* s) {
        WLK_HIP(hipEventRecord(joined[r], s->stream));
        WLK_HIP(hipStreamWaitEvent(stream, joined[r], 0));
    }
    void stacked_ws_ready();             // the stacked decoder pass's workspace, allocated by the first call that needs it
    int run_pick(wlk_session* const* sessions, const int64_t* tokens, const wlk_pick_params* p, const int32_t* max_steps, int n,
                 int burst, int32_t* tokens_out, float* logprobs_out, int32_t* steps_out);
};

// The host checks of one listed session that every entry point makes before anything is launched (a refused call touches
// nothing), in the order each entry point has always made them.  own_arg_error: the verdict on the row's other arguments,
// which ranks behind the session's own argument errors and before its state.  The stacked decoder pass of an alignment or
// a verify call takes plain sessions only; a verify pass, as a prefill, none that keeps raw alignment scores.
enum GateCall { kGateStep, kGateAlign, kGateVerify };
static int gate_session(const wlk_group* g, const wlk_session* s, bool listed_before, GateCall call,
                        const char* own_arg_error = nullptr) {
    static const char* const kName[] = {"window group step", "find_alignment", "verify"};
    const char* name = kName[call];
    if (!s) return fail(WLK_ERR_ARG, "window group: NULL session");
    if (listed_before) return fail(WLK_ERR_ARG, "window group: a session is listed twice");
    if (s->m != g->m) return fail(WLK_ERR_ARG, "window group: a session of another model");
    if (s->beam != 1) return fail(WLK_ERR_ARG, std::string(name) + " needs a beam-1 session");
    if (own_arg_error) return fail(WLK_ERR_ARG, own_arg_error);
    if (s->engine) return fail(WLK_ERR_STATE, "window group: the session is attached to the batch engine");
    if (!s->encoded) return fail(WLK_ERR_STATE, std::string(name) + " before an encode");
    if (call == kGateVerify && !s->rules_mask) return fail(WLK_ERR_STATE, "verify before wlk_rules_set");
    if (call != kGateStep && (s->debug || s->prof_on || (call == kGateVerify && (s->align_raw_scores || s->survey))))
        return fail(WLK_ERR_STATE, "window group: not a plain beam-1 session");
    return WLK_OK;
}
// the stacked pass overwrites the session's caches and score window: whatever happens from there on, its next decode must be
// a prefill (as after wlk_find_alignment)
static void next_decode_is_prefill(wlk_session* s) {
    s->n_steps = 0;
    s->self_len = 0;
    s->have_sot = false;
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
        wlk_step_ws_alloc(m, g->ws);
        g->blk_dev = reinterpret_cast<GroupBlock*>(dev_alloc<char>(sizeof(GroupBlock)));
        g->pick_dev = dev_alloc<int>(2 * kGroupMaxRows);
        g->results_dev = reinterpret_cast<GroupResults*>(dev_alloc<char>(sizeof(GroupResults)));
        WLK_HIP(hipHostMalloc(reinterpret_cast<void**>(&g->pinned), sizeof(GroupBlock) + sizeof(GroupResults), hipHostMallocDefault));
        std::memset(g->pinned, 0, sizeof(GroupBlock) + sizeof(GroupResults));
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
    return g->run_pick(sessions, tokens, p, nullptr, n, 1, tokens_out, logprobs_out, nullptr);
}

int wlk_group_run_pick(wlk_group* g, wlk_session* const* sessions, const int64_t* tokens, const wlk_pick_params* p,
                       const int32_t* max_steps, int n, int burst, int32_t* tokens_out, float* logprobs_out, int32_t* steps_out) {
    if (!g || !sessions || !tokens || !p || !max_steps || !tokens_out || !logprobs_out || !steps_out)
        return fail(WLK_ERR_ARG, "NULL argument");
    return g->run_pick(sessions, tokens, p, max_steps, n, burst, tokens_out, logprobs_out, steps_out);
}

}  // extern "C"

// Up to `burst` single-token steps of n sessions behind one upload, one read-back and one synchronisation: the body of
// wlk_group_step_pick (max_steps == nullptr: one step of every row, results [n]) and of wlk_group_run_pick (results
// [n][burst], entries behind a row's last own step untouched).
int wlk_group::run_pick(wlk_session* const* sessions, const int64_t* tokens, const wlk_pick_params* p, const int32_t* max_steps,
                        int n, int burst, int32_t* tokens_out, float* logprobs_out, int32_t* steps_out) {
    wlk_group* g = this;
    if (n < 1 || n > g->max_rows) return fail(WLK_ERR_ARG, "window group: 1..max_rows sessions per step");
    if (burst < 1 || burst > kGroupMaxBurst) return fail(WLK_ERR_ARG, "window group: 1..16 steps per call");
    const wlk_dims& D = g->m->D;
    // every session is checked on the host before anything is launched: a refused call has advanced nobody
    for (int r = 0; r < n; ++r) {
        const wlk_session* s = sessions[r];
        const char* own = tokens[r] < 0 || tokens[r] >= D.n_vocab ? "token id out of range"
                          : !pick_params_ok(p[r], D.n_vocab)      ? "rule parameters out of range"
                          : max_steps && max_steps[r] < 1         ? "window group: a row's step budget is at least 1"
                                                                  : nullptr;
        if (const int rc = gate_session(g, s, std::find(sessions, sessions + r, s) != sessions + r, kGateStep, own)) return rc;
        if (s->n_steps < 1) return fail(WLK_ERR_STATE, "window group: step before the session's prefill");
        if (!s->rules_mask) return fail(WLK_ERR_STATE, "window group: step before wlk_rules_set");
        if (s->self_len + 1 > D.n_text_ctx) return fail(WLK_ERR_STATE, "text context exceeded");
    }
    return guarded([&]() {
        std::lock_guard<std::mutex> lk(g->mu);
        WLK_HIP(hipSetDevice(g->m->device));
        GroupBlock* blk = reinterpret_cast<GroupBlock*>(g->pinned);
        GroupResults* res = reinterpret_cast<GroupResults*>(g->pinned + sizeof(GroupBlock));
        for (int r = 0; r < n; ++r) {
            wlk_session* s = sessions[r];
            blk->rows[r] = next_step_row(s, (int)tokens[r], D.n_audio_ctx);
            blk->pick[r] = PickRowEntry{s->rules_mask, pick_rules_of(p[r])};
            const int limit = std::min(std::min(max_steps ? (int)max_steps[r] : 1, burst), (int)D.n_text_ctx - s->self_len);
            blk->burst[r] = BurstRow{1, 0, limit, s->n_steps, s->self_len, s->prefill_rows};
            g->join(r, s);
        }
        uint64_t rows_taken = 0;
        if (burst == 1) {
            // one chain: the pick slots are the results and nothing has to be advanced on the device
            const size_t up = offsetof(GroupBlock, pick) + (size_t)n * sizeof(PickRowEntry);
            WLK_HIP(hipMemcpyAsync(g->blk_dev, blk, up, hipMemcpyHostToDevice, g->stream));
            g->enqueue_step(n);
            WLK_HIP(hipMemcpyAsync(res->picks, g->pick_dev, (size_t)8 * n, hipMemcpyDeviceToHost, g->stream));
            WLK_HIP(hipStreamSynchronize(g->stream));
        } else {
            const size_t up = offsetof(GroupBlock, burst) + (size_t)n * sizeof(BurstRow);
            WLK_HIP(hipMemcpyAsync(g->blk_dev, blk, up, hipMemcpyHostToDevice, g->stream));
            for (int k = 0; k < burst; ++k) {      // nothing from the host goes between the chains
                g->enqueue_step(n);
                hipLaunchKernelGGL(group_advance_rows_kernel, dim3(1), dim3(64), 0, g->stream, g->blk_dev, g->pick_dev,
                                   g->results_dev, n, (int)D.n_text_ctx);
                WLK_HIP(hipGetLastError());
            }
            WLK_HIP(hipMemcpyAsync(res, g->results_dev, sizeof(GroupResults), hipMemcpyDeviceToHost, g->stream));
            WLK_HIP(hipStreamSynchronize(g->stream));
            for (int r = 0; r < n; ++r)
                if (res->taken[r] < 1 || res->taken[r] > blk->burst[r].limit)
                    throw std::logic_error("window group: a row's step count is out of range");
        }
        for (int r = 0; r < n; ++r) {
            wlk_session* s = sessions[r];
            int steps = 1;
            if (burst == 1) {
                const int* one = &res->picks[0][0][0] + 2 * r;     // the pick slots, [n][2]
                tokens_out[r] = one[0];
                std::memcpy(&logprobs_out[r], &one[1], 4);
            } else {
                steps = res->taken[r];
                for (int k = 0; k < steps; ++k) {
                    tokens_out[(size_t)r * burst + k] = res->picks[r][k][0];
                    std::memcpy(&logprobs_out[(size_t)r * burst + k], &res->picks[r][k][1], 4);
                }
            }
            if (steps_out) steps_out[r] = steps;
            s->self_len += steps;
            s->n_steps += steps;
            s->have_sot = false;
            s->last_rows = 1;
            s->last_ntok = 1;
            rows_taken += (uint64_t)steps;
        }
        g->last_rows = n;
        g->n_steps += (uint64_t)burst;       // chains enqueued
        g->n_rows += rows_taken;             // row-steps taken: the rest of burst x n went to rows that had ended
        return WLK_OK;
    });
}

// ---- stacked word alignment ----------------------------------------------------------------------------------
namespace {
constexpr int kAlignRowsMax = 256;       // longest token sequence of one window in the stacked pass
constexpr size_t kAlignUpBytes = sizeof(AlignWin) * kGroupMaxRows + sizeof(int) * kGroupMaxRows * kAlignRowsMax;
constexpr size_t kAlignResBytes = sizeof(int) * 2 * kGroupMaxRows * kAlignRowsMax;
inline size_t up16(size_t n) { return (n + 15) / 16 * 16; }

int align_session_rows(const wlk_model* m) { return std::min(kAlignRowsMax, (int)m->D.n_text_ctx); }

// the shape conditions of a window in the stacked pass: a pure host function of (model, P, num_frames); empty = fits
std::string align_shape_refusal(const wlk_model* m, int P, int num_frames) {
    const int F = num_frames / 2;
    if (m->n_align < 1) return "the model has no alignment heads";
    if (F < 1 || F > m->D.n_audio_ctx) return "num_frames out of range";
    return wlk_prefill_shape_check(m, P, align_session_rows(m));
}
}  // namespace

void wlk_group::stacked_ws_ready() {
    if (align_ready) return;
    wlk_prefill_ws_alloc(m, align_ws, kGroupMaxRows, align_session_rows(m));
    align_ready = true;
}

extern "C" {

int wlk_group_align_fits(wlk_group* g, int32_t n_tokens, int32_t num_frames, int32_t* fits) {
    if (!g || !fits) return fail(WLK_ERR_ARG, "NULL argument");
    *fits = align_shape_refusal(g->m, n_tokens, num_frames).empty() ? 1 : 0;
    return WLK_OK;
}

int wlk_group_find_alignment(wlk_group* g, const wlk_align_window* w, int n) {
    if (!g || !w) return fail(WLK_ERR_ARG, "NULL argument");
    if (n < 1 || n > g->max_rows) return fail(WLK_ERR_ARG, "window group: 1..max_rows windows per alignment pass");
    wlk_model* m = g->m;
    const wlk_dims& D = m->D;
    // every window is checked on the host before anything is launched or any session is touched
    for (int r = 0; r < n; ++r) {
        const wlk_align_window& a = w[r];
        const wlk_session* s = a.s;
        if (!s || !a.tokens || !a.starts || !a.token_probs) return fail(WLK_ERR_ARG, "window group: NULL argument in an alignment window");
        const bool twice = std::any_of(w, w + r, [s](const wlk_align_window& o) { return o.s == s; });
        if (const int rc = gate_session(g, s, twice, kGateAlign)) return rc;
        const int P = a.n_tokens, n_text = P - a.n_sot - 2;
        if (a.n_sot < 1 || n_text < 1) return fail(WLK_ERR_ARG, "find_alignment: need [sot sequence, notimestamps, >= 1 text token, eot]");
        if (a.eot < 1 || a.eot > D.n_vocab) return fail(WLK_ERR_ARG, "find_alignment: eot out of range");
        const std::string shape = align_shape_refusal(m, P, a.num_frames);
        if (!shape.empty()) return fail(WLK_ERR_ARG, "find_alignment: " + shape);
        for (int i = 0; i < P; ++i)
            if (a.tokens[i] < 0 || a.tokens[i] >= D.n_vocab) return fail(WLK_ERR_ARG, "token id out of range");
        for (int i = 0; i < n_text; ++i)
            if (a.tokens[a.n_sot + 1 + i] >= a.eot) return fail(WLK_ERR_ARG, "find_alignment: text token >= eot");
    }
    return guarded([&]() {
        std::lock_guard<std::mutex> lk(g->mu);
        WLK_HIP(hipSetDevice(m->device));
        const LaunchCtx c{g->stream, nullptr};
        const int d = D.n_text_state, T = D.n_audio_ctx;
        g->stacked_ws_ready();
        if (!g->align_up_dev) {
            g->align_up_dev = dev_alloc<char>(kAlignUpBytes);
            WLK_HIP(hipHostMalloc(reinterpret_cast<void**>(&g->align_pinned), kAlignUpBytes + kAlignResBytes, hipHostMallocDefault));
        }
        // ---- workspace: [hidden max n_text x d | logits max n_text x eot | per window: w, cost | results | trace_t | trace]
        size_t hid_b = 0, log_b = 0, wc_b = 0, tr_b = 0, n_res = 0;
        for (int r = 0; r < n; ++r) {
            const int P = w[r].n_tokens, n_text = P - w[r].n_sot - 2, N = n_text + 1, F = w[r].num_frames / 2;
            hid_b = std::max(hid_b, up16((size_t)n_text * d * 4));
            log_b = std::max(log_b, up16((size_t)n_text * w[r].eot * 4));
            wc_b += up16((size_t)m->n_align * P * F * 4) + up16((size_t)N * F * 4);
            tr_b += up16((size_t)(N + 1) * (F + 1));
            n_res += (size_t)N + n_text;
        }
        const size_t res_b = up16(n_res * 4);
        g->align_buf.reserve(hid_b + log_b + wc_b + res_b + 2 * tr_b, g->stream);
        float* hid = reinterpret_cast<float*>(g->align_buf.p);
        float* logits = reinterpret_cast<float*>(g->align_buf.p + hid_b);
        char* at = g->align_buf.p + hid_b + log_b;
        int* res_dev = reinterpret_cast<int*>(at + wc_b);
        signed char* trace_t0 = reinterpret_cast<signed char*>(at + wc_b + res_b);
        signed char* trace0 = trace_t0 + tr_b;

        // ---- tables: one AlignWin per window, the text tokens as the probability targets; results = [starts | probs] of
        // window 0, then of window 1, ...
        AlignWin* tab_h = reinterpret_cast<AlignWin*>(g->align_pinned);
        int* tgt_h = reinterpret_cast<int*>(g->align_pinned + sizeof(AlignWin) * kGroupMaxRows);
        AlignWin* tab_dev = reinterpret_cast<AlignWin*>(g->align_up_dev);
        int* tgt_dev = reinterpret_cast<int*>(g->align_up_dev + sizeof(AlignWin) * kGroupMaxRows);
        int* res_h = reinterpret_cast<int*>(g->align_pinned + kAlignUpBytes);
        std::vector<wlk_prefill_item> items(n);
        std::vector<wlk_prefill_item*> stack(n);
        std::vector<size_t> res_at(n), tgt_at(n);
        size_t tr_at = 0, r_at = 0, t_at = 0;
        for (int r = 0; r < n; ++r) {
            wlk_session* s = w[r].s;
            const int P = w[r].n_tokens, n_sot = w[r].n_sot, n_text = P - n_sot - 2, N = n_text + 1, F = w[r].num_frames / 2;
            AlignWin& t = tab_h[r];
            t = AlignWin{};
            t.ring = s->ring;
            t.w = reinterpret_cast<float*>(at);
            at += up16((size_t)m->n_align * P * F * 4);
            t.cost = reinterpret_cast<float*>(at);
            at += up16((size_t)N * F * 4);
            t.trace_t = trace_t0 + tr_at;
            t.trace = trace0 + tr_at;
            tr_at += up16((size_t)(N + 1) * (F + 1));
            t.starts = res_dev + r_at;
            res_at[r] = r_at;
            r_at += (size_t)N + n_text;
            t.P = P; t.F = F; t.n_sot = n_sot; t.N = N; t.qk_scale = w[r].qk_scale;
            tgt_at[r] = t_at;
            for (int i = 0; i < n_text; ++i) tgt_h[t_at + i] = (int)w[r].tokens[n_sot + 1 + i];
            t_at += n_text;
            items[r].s = s; items[r].tokens = w[r].tokens; items[r].n_tok = P; items[r].sot_index = 0;
            stack[r] = &items[r];
            if (s->ring_rows != w[0].s->ring_rows) throw std::logic_error("window group: score windows of different heights");
            next_decode_is_prefill(s);
            g->join(r, s);
        }
        WLK_HIP(hipMemcpyAsync(g->align_up_dev, g->align_pinned, kAlignUpBytes, hipMemcpyHostToDevice, g->stream));

        // ---- ONE decoder pass over the rows of all windows; raw alignment scores land in each session's score window
        std::vector<int> row0;
        wlk_prefill_chain(stack, c, g->align_ws, row0);
        // ---- token probabilities, per window with the solo call's launches (M = n_text is compute-bound: stacking the rows
        // would buy nothing and change the kernel choice) into one reused logits buffer
        for (int r = 0; r < n; ++r) {
            const int n_sot = w[r].n_sot, n_text = w[r].n_tokens - n_sot - 2, eot = w[r].eot;
            launch_layernorm(c, g->align_ws.dx + (size_t)(row0[r] + n_sot) * d, d, m->w_ln_w, m->w_ln_b, hid, d, n_text, d, "wa_ln_f");
            GemmArgs lg;
            lg.A = hid; lg.lda = d; lg.W = m->w_tok_emb; lg.C = logits; lg.ldc = eot; lg.M = n_text; lg.N = eot; lg.K = d;
            launch_linear(c, lg, "wa_logits");
            launch_wa_token_prob(c, logits, eot, eot, tgt_dev + tgt_at[r],
                                 reinterpret_cast<float*>(res_dev + res_at[r] + n_text + 1), n_text);
        }
        // ---- attention -> cost matrices -> warping -> path walk: six launches for all windows
        launch_word_align_ragged(c, tab_dev, tab_h, n, m->n_align, w[0].s->ring_rows, T);
        WLK_HIP(hipMemsetAsync(trace_t0, 0xff, tr_at, g->stream));   // -1 like dtw_cpu's untouched border cells
        launch_dtw_ragged(c, tab_dev, tab_h, n);
        WLK_HIP(hipMemcpyAsync(res_h, res_dev, r_at * sizeof(int), hipMemcpyDeviceToHost, g->stream));
        WLK_HIP(hipStreamSynchronize(g->stream));
        for (int r = 0; r < n; ++r) {
            const int n_text = w[r].n_tokens - w[r].n_sot - 2, N = n_text + 1, F = w[r].num_frames / 2;
            std::memcpy(w[r].starts, res_h + res_at[r], (size_t)N * sizeof(int));
            std::memcpy(w[r].token_probs, res_h + res_at[r] + N, (size_t)n_text * sizeof(float));
            // tests only (host buffers are the caller's: pageable, so synchronous)
            if (w[r].cost) copy_sync(w[r].cost, tab_h[r].cost, (size_t)N * F * sizeof(float), hipMemcpyDeviceToHost);
            if (w[r].trace) copy_sync(w[r].trace, tab_h[r].trace, (size_t)(N + 1) * (F + 1), hipMemcpyDeviceToHost);
        }
        return WLK_OK;
    });
}

}  // extern "C"

// ---- draft verification --------------------------------------------------------------------------------------
namespace {
constexpr int kVerifyResInts = 8;        // per window: accepted, next token, its log-probability, the sum, no-speech probability
constexpr size_t kVerifyDraftInts = (size_t)kGroupMaxRows * kMaxDraft;
constexpr size_t kVerifyPickInts = (size_t)kGroupMaxRows * (kMaxDraft + 1) * 3;
constexpr size_t kVerifyResAll = (size_t)kGroupMaxRows * kVerifyResInts;

// the shape conditions of a window in the verify pass: a pure host function of (model, P0, n_d); empty = fits
std::string verify_shape_refusal(const wlk_model* m, int n_initial, int n_draft) {
    if (n_initial < 1) return "no initial tokens";
    if (n_draft < 1) return "an empty draft";
    if (n_draft > kMaxDraft || n_initial > kAlignRowsMax) return "prompt length outside the stacked range";
    const int P = n_initial + n_draft;
    if (P > m->D.n_text_ctx) return "text context exceeded";
    return wlk_prefill_shape_check(m, P, align_session_rows(m));
}
}  // namespace

extern "C" {

int wlk_group_verify_fits(wlk_group* g, int32_t n_initial, int32_t n_draft, int32_t* fits) {
    if (!g || !fits) return fail(WLK_ERR_ARG, "NULL argument");
    *fits = verify_shape_refusal(g->m, n_initial, n_draft).empty() ? 1 : 0;
    return WLK_OK;
}

int wlk_group_verify(wlk_group* g, const wlk_verify_window* w, int n) {
    if (!g || !w) return fail(WLK_ERR_ARG, "NULL argument");
    if (n < 1 || n > g->max_rows) return fail(WLK_ERR_ARG, "window group: 1..max_rows windows per verify pass");
    wlk_model* m = g->m;
    const wlk_dims& D = m->D;
    const int V = D.n_vocab;
    // every window is checked on the host before anything is launched or any session is touched
    for (int r = 0; r < n; ++r) {
        const wlk_verify_window& a = w[r];
        const wlk_session* s = a.s;
        if (!s || !a.tokens || !a.result) return fail(WLK_ERR_ARG, "window group: NULL argument in a verify window");
        const bool twice = std::any_of(w, w + r, [s](const wlk_verify_window& o) { return o.s == s; });
        if (const int rc = gate_session(g, s, twice, kGateVerify)) return rc;
        const int P0 = a.n_initial, P = a.n_tokens, n_d = P - P0;
        if (n_d < 1) return fail(WLK_ERR_ARG, "verify: an empty draft");
        const std::string shape = verify_shape_refusal(m, P0, n_d);
        if (!shape.empty()) return fail(WLK_ERR_ARG, "verify: " + shape);
        if (a.sot_index < 0 || a.sot_index >= P0) return fail(WLK_ERR_ARG, "sot_index out of range");
        if (!pick_params_ok(a.p, V)) return fail(WLK_ERR_ARG, "rule parameters out of range");
        if (a.no_speech_token >= V) return fail(WLK_ERR_ARG, "token out of range");
        for (int i = 0; i < P; ++i)
            if (a.tokens[i] < 0 || a.tokens[i] >= V) return fail(WLK_ERR_ARG, "token id out of range");
        for (int i = P0; i < P; ++i)
            if (a.tokens[i] == a.p.eot) return fail(WLK_ERR_ARG, "verify: <|endoftext|> inside the draft");
        if (s->ring_rows < P) return fail(WLK_ERR_ARG, "verify: the session's score window is shorter than the pass");
        if (s->ring_rows != w[0].s->ring_rows) return fail(WLK_ERR_ARG, "window group: score windows of different heights");
    }
    return guarded([&]() {
        std::lock_guard<std::mutex> lk(g->mu);
        WLK_HIP(hipSetDevice(m->device));
        const LaunchCtx c{g->stream, nullptr};
        const int d = D.n_text_state, T = D.n_audio_ctx;
        g->stacked_ws_ready();
        if (!g->verify_dev) {
            g->verify_dev = dev_alloc<int>(kVerifyDraftInts + kVerifyPickInts + kVerifyResAll);
            WLK_HIP(hipHostMalloc(reinterpret_cast<void**>(&g->verify_pinned), (kVerifyDraftInts + kVerifyResAll) * sizeof(int),
                                  hipHostMallocDefault));
        }
        // ---- workspace: [hidden | logits] of the longest window: its n_d + 1 candidate rows and the sot row behind them
        int rows_max = 0;
        for (int r = 0; r < n; ++r) rows_max = std::max(rows_max, w[r].n_tokens - w[r].n_initial + 2);
        const size_t hid_b = up16((size_t)rows_max * d * 4);
        g->verify_buf.reserve(hid_b + up16((size_t)rows_max * V * 4), g->stream);
        float* hid = reinterpret_cast<float*>(g->verify_buf.p);
        float* logits = reinterpret_cast<float*>(g->verify_buf.p + hid_b);
        int* draft_dev = g->verify_dev;
        int* picks_dev = draft_dev + kVerifyDraftInts;
        int* res_dev = picks_dev + kVerifyPickInts;
        int* draft_h = g->verify_pinned;
        int* res_h = draft_h + kVerifyDraftInts;

        std::vector<wlk_prefill_item> items(n);
        std::vector<wlk_prefill_item*> stack(n);
        for (int r = 0; r < n; ++r) {
            wlk_session* s = w[r].s;
            const int P0 = w[r].n_initial, n_d = w[r].n_tokens - P0;
            for (int i = 0; i < n_d; ++i) draft_h[(size_t)r * kMaxDraft + i] = (int)w[r].tokens[P0 + i];
            items[r].s = s; items[r].tokens = w[r].tokens; items[r].n_tok = w[r].n_tokens; items[r].sot_index = w[r].sot_index;
            stack[r] = &items[r];
            next_decode_is_prefill(s);
            g->join(r, s);
        }
        WLK_HIP(hipMemcpyAsync(draft_dev, draft_h, (size_t)n * kMaxDraft * sizeof(int), hipMemcpyHostToDevice, g->stream));
        WLK_HIP(hipMemsetAsync(res_dev, 0, kVerifyResAll * sizeof(int), g->stream));

        // ---- ONE teacher-forced decoder pass over [initial | draft] of all windows.  It writes K/V rows 0 .. P - 1 of every
        // session.  Of those, rows at and behind P0 + k (k = the accepted count) belong to draft tokens greedy decoding would
        // not have produced; they stay where they are, stale: a step at offset o reads the cache positions below o and
        // writes position o (the argument of group_advance_rows_kernel's dead rows and of the padded tile rows),
        // and the session goes on at offset P0 + k - so every stale row is overwritten by the step that owns its position
        // before any step reads it.  Rows below P0 + k depend on tokens below P0 + k only (causal self-attention, row-wise
        // operators elsewhere): they are the rows a prefill of [initial | draft[0 .. k)] writes.
        std::vector<int> row0;
        wlk_prefill_chain(stack, c, g->align_ws, row0);
        for (int r = 0; r < n; ++r) {
            wlk_session* s = w[r].s;
            const int P0 = w[r].n_initial, P = w[r].n_tokens, n_d = P - P0, n_pos = n_d + 1;
            // the alignment heads' raw scores softmaxed in place, as a prefill leaves them (row-wise: rows below P0 + k are
            // those of the shorter prefill)
            if (m->n_align > 0)
                launch_ring_softmax(c, s->ring, g->align_ws.ring_row_dev + row0[r], g->align_ws.zeros_dev, m->all_ranks, m->n_align, P,
                                    s->ring_rows, 1, T);
            // ---- final LayerNorm of the candidate rows P0 - 1 .. P - 1 and of the sot row, projected onto the vocabulary
            // by one launch into the reused logits buffer (rows 0 .. n_d: the candidates; row n_d + 1: the sot row)
            const float* x0 = g->align_ws.dx + (size_t)row0[r] * d;
            launch_layernorm(c, x0 + (size_t)(P0 - 1) * d, d, m->w_ln_w, m->w_ln_b, hid, d, n_pos, d, "dv_ln_f");
            launch_layernorm(c, x0 + (size_t)w[r].sot_index * d, d, m->w_ln_w, m->w_ln_b, hid + (size_t)n_pos * d, d, 1, d, "dv_ln_f");
            GemmArgs lg;
            lg.A = hid; lg.lda = d; lg.W = m->w_tok_emb; lg.C = logits; lg.ldc = V; lg.M = n_pos + 1; lg.N = V; lg.K = d;
            launch_linear(c, lg, "dv_logits");
            int* res = res_dev + (size_t)r * kVerifyResInts;
            if (w[r].no_speech_token >= 0)
                launch_token_prob(c, logits + (size_t)n_pos * V, V, 1, w[r].no_speech_token, reinterpret_cast<float*>(res + 4));
            const int ended = w[r].tokens[P0 - 1] == w[r].p.eot ? 1 : 0;
            launch_draft_pick(c, logits, V, s->rules_mask, pick_rules_of(w[r].p), draft_dev + (size_t)r * kMaxDraft, n_d, ended,
                              picks_dev + (size_t)r * (kMaxDraft + 1) * 3, res, s->logits_last);
            WLK_HIP(hipMemcpyAsync(s->logits_sot, logits + (size_t)n_pos * V, (size_t)V * sizeof(float), hipMemcpyDeviceToDevice,
                                   g->stream));
        }
        WLK_HIP(hipMemcpyAsync(res_h, res_dev, (size_t)n * kVerifyResInts * sizeof(int), hipMemcpyDeviceToHost, g->stream));
        WLK_HIP(hipStreamSynchronize(g->stream));
        for (int r = 0; r < n; ++r) {
            const int n_d = w[r].n_tokens - w[r].n_initial;
            if (res_h[r * kVerifyResInts] < 0 || res_h[r * kVerifyResInts] > n_d)
                throw std::logic_error("window group: an accepted count is out of range");
        }
        for (int r = 0; r < n; ++r) {
            const wlk_verify_window& o = w[r];
            wlk_session* s = o.s;
            const int* res = res_h + (size_t)r * kVerifyResInts;
            const int P0 = o.n_initial, n_d = o.n_tokens - P0, k = res[0];
            o.result->accepted = k;
            o.result->next_token = res[1];
            std::memcpy(&o.result->next_logprob, &res[2], 4);
            std::memcpy(&o.result->sum_logprob, &res[3], 4);
            if (o.no_speech_token >= 0) std::memcpy(&o.result->no_speech_prob, &res[4], 4);
            else o.result->no_speech_prob = NAN;
            // tests only (the host buffer is the caller's: pageable, so synchronous)
            if (o.picks) {
                std::vector<int> pk((size_t)(n_d + 1) * 3);
                copy_sync(pk.data(), picks_dev + (size_t)r * (kMaxDraft + 1) * 3, pk.size() * sizeof(int), hipMemcpyDeviceToHost);
                for (int j = 0; j <= n_d; ++j) {
                    o.picks[2 * j] = pk[3 * j];
                    o.picks[2 * j + 1] = pk[3 * j + 1];
                }
            }
            // the session is what a prefill of [initial | draft[0 .. k)] leaves
            s->self_len = P0 + k;
            s->n_steps = 1;
            s->have_sot = true;
            s->prefill_rows = P0 + k;
            s->last_rows = 1;
            s->last_ntok = P0 + k;
            s->anc_live = false;
        }
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
        copy_sync(host, g->ws.logits + (size_t)row * V, V * sizeof(float), hipMemcpyDeviceToHost);
        return WLK_OK;
    });
}

// The logits and the masks of the pick entries below (wlk_diag_pick_rows, _pick_one, _pick_topk, _draft_pick) are followed by
// one guard entry each - a logit of +inf under a mask byte that allows it: a sweep that reads one entry past the last row
// picks token n_vocab, which no reference names.
static void upload_guarded(DevBytes& d, const void* host, size_t bytes, const void* guard, size_t guard_bytes) {
    d.alloc(bytes + guard_bytes);
    WLK_HIP(hipMemcpy(d.p, host, bytes, hipMemcpyHostToDevice));
    WLK_HIP(hipMemcpy(d.p + bytes, guard, guard_bytes, hipMemcpyHostToDevice));
}
static void upload_guarded_row(DevBytes& logits, const float* logits_host, size_t n_floats, DevBytes& mask, const uint8_t* mask_host,
                               size_t mask_bytes) {
    const float inf = INFINITY;
    const uint8_t allow = 0;
    upload_guarded(logits, logits_host, n_floats * sizeof(float), &inf, sizeof(float));
    upload_guarded(mask, mask_host, mask_bytes, &allow, 1);
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
        DevBytes logits, masks, out(8 * n);
        upload_guarded_row(logits, logits_host, V * n, masks, masks_host, V * n_masks);
        PickRowEntry host[kGroupMaxRows];
        for (int r = 0; r < n; ++r) host[r] = PickRowEntry{masks.as<unsigned char>() + V * mask_of_row[r], pick_rules_of(p[r])};
        DevBytes table(sizeof(PickRowEntry) * n, host);
        launch_rules_pick_rows(LaunchCtx{nullptr, nullptr}, logits.f(), n_vocab, n, table.as<PickRowEntry>(), out.i());
        int res[2 * kGroupMaxRows];
        WLK_HIP(hipStreamSynchronize(nullptr));
        out.back(res);
        for (int r = 0; r < n; ++r) {
            tokens_out[r] = res[2 * r];
            std::memcpy(&logprobs_out[r], &res[2 * r + 1], 4);
        }
        return WLK_OK;
    });
}

// Tests: rules_pick_kernel, the one-row pick behind wlk_pick_greedy, on one host logits row, one rule mask and one parameter
// block.  logprob_bits_out receives the bits of the float the kernel wrote.
int wlk_diag_pick_one(const float* logits_host, int n_vocab, const uint8_t* mask_host, const wlk_pick_params* p, int32_t* token_out,
                      uint32_t* logprob_bits_out) {
    if (!logits_host || !mask_host || !p || !token_out || !logprob_bits_out) return fail(WLK_ERR_ARG, "NULL argument");
    if (n_vocab < 1) return fail(WLK_ERR_ARG, "pick one: n_vocab >= 1");
    if (!pick_params_ok(*p, n_vocab)) return fail(WLK_ERR_ARG, "pick one: rule parameters out of range");
    return guarded([&]() {
        const size_t V = (size_t)n_vocab;
        DevBytes logits, mask, out(8);
        upload_guarded_row(logits, logits_host, V, mask, mask_host, V);
        launch_rules_pick(LaunchCtx{nullptr, nullptr}, logits.f(), n_vocab, mask.as<unsigned char>(), pick_rules_of(*p), out.i(),
                          reinterpret_cast<float*>(out.i() + 1));
        int res[2];
        WLK_HIP(hipStreamSynchronize(nullptr));
        out.back(res);
        token_out[0] = res[0];
        std::memcpy(logprob_bits_out, &res[1], 4);
        return WLK_OK;
    });
}

// Tests: rules_topk_kernel, the rules + log-softmax + k best behind wlk_pick_topk, on host logits [n_rows][n_vocab], one rule
// mask and one parameter block per row.  logprobs_out / ids_out [n_rows][k].
int wlk_diag_pick_topk(const float* logits_host, int n_vocab, const uint8_t* mask_host, const wlk_pick_params* p, int n_rows, int k,
                       float* logprobs_out, int32_t* ids_out) {
    if (!logits_host || !mask_host || !p || !logprobs_out || !ids_out) return fail(WLK_ERR_ARG, "NULL argument");
    if (n_rows < 1 || n_rows > kMaxPickRows || k < 1 || k > 8 || n_vocab < 1) return fail(WLK_ERR_ARG, "pick top-k: 1..8 rows, k in [1, 8]");
    for (int r = 0; r < n_rows; ++r)
        if (!pick_params_ok(p[r], n_vocab)) return fail(WLK_ERR_ARG, "pick top-k: rule parameters out of range");
    return guarded([&]() {
        const size_t V = (size_t)n_vocab, n_out = (size_t)n_rows * k;
        DevBytes logits, mask, out(8 * n_out);   // [log-probs | ids]
        upload_guarded_row(logits, logits_host, V * n_rows, mask, mask_host, V);
        PickRulesRows rules{};
        for (int r = 0; r < n_rows; ++r) rules.r[r] = pick_rules_of(p[r]);
        launch_rules_topk(LaunchCtx{nullptr, nullptr}, logits.f(), n_vocab, n_rows, mask.as<unsigned char>(), rules, k, out.f(),
                          out.i() + n_out);
        std::vector<int> host(2 * n_out);
        WLK_HIP(hipStreamSynchronize(nullptr));
        out.back(host.data());
        std::memcpy(logprobs_out, host.data(), 4 * n_out);
        std::memcpy(ids_out, host.data() + n_out, 4 * n_out);
        return WLK_OK;
    });
}

// Tests: the device form of the rule transition alone (pick_rules_advance), out[i] = the state after tokens[i] was picked
// under p[i].  No model, any n >= 1.
int wlk_diag_pick_advance(const wlk_pick_params* p, const int32_t* tokens, int n, wlk_pick_params* out) {
    if (!p || !tokens || !out) return fail(WLK_ERR_ARG, "NULL argument");
    if (n < 1) return fail(WLK_ERR_ARG, "pick advance: n >= 1");
    return guarded([&]() {
        std::vector<PickRules> host(n);
        for (int i = 0; i < n; ++i) host[i] = pick_rules_of(p[i]);
        DevBytes in_dev(sizeof(PickRules) * n, host.data()), out_dev(sizeof(PickRules) * n), tok_dev(sizeof(int) * (size_t)n, tokens);
        hipLaunchKernelGGL(pick_advance_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, in_dev.as<const PickRules>(),
                           tok_dev.as<const int>(), n, out_dev.as<PickRules>());
        WLK_HIP(hipGetLastError());
        WLK_HIP(hipStreamSynchronize(nullptr));
        out_dev.back(host.data());
        for (int i = 0; i < n; ++i) {
            const PickRules& q = host[i];
            out[i] = wlk_pick_params{q.first_step, q.without_timestamps, q.timestamp_begin, q.eot, q.no_timestamps, q.ts_mode,
                                     q.ts_bound, q.max_initial};
        }
        return WLK_OK;
    });
}

// Tests: the two kernels behind wlk_group_verify's decoder pass alone (select.hip: draft_pick_rows_kernel,
// draft_accept_kernel) on host logits [n_draft + 1][n_vocab], one rule mask [n_vocab] and the first-pick state p0.
int wlk_diag_draft_pick(const float* logits_host, int n_vocab, const uint8_t* mask_host, const wlk_pick_params* p0,
                        const int32_t* draft, int n_draft, int ended, int32_t* tokens_out, float* logprobs_out,
                        wlk_verify_result* result) {
    if (!logits_host || !mask_host || !p0 || !draft || !tokens_out || !logprobs_out || !result) return fail(WLK_ERR_ARG, "NULL argument");
    if (n_draft < 1 || n_draft > kMaxDraft || n_vocab < 1) return fail(WLK_ERR_ARG, "draft pick: 1..256 draft tokens");
    if (!pick_params_ok(*p0, n_vocab)) return fail(WLK_ERR_ARG, "draft pick: rule parameters out of range");
    return guarded([&]() {
        const size_t V = (size_t)n_vocab, n_pos = (size_t)n_draft + 1;
        DevBytes logits, mask, drafts(sizeof(int) * (size_t)n_draft, draft), picks((n_pos * 3 + 4) * sizeof(int));   // [picks n_pos x 3 | result 4]
        upload_guarded_row(logits, logits_host, V * n_pos, mask, mask_host, V);
        launch_draft_pick(LaunchCtx{nullptr, nullptr}, logits.f(), n_vocab, mask.as<unsigned char>(), pick_rules_of(*p0), drafts.i(),
                          n_draft, ended ? 1 : 0, picks.i(), picks.i() + n_pos * 3, nullptr);
        WLK_HIP(hipStreamSynchronize(nullptr));
        std::vector<int> host(n_pos * 3 + 4);
        picks.back(host.data());
        for (size_t j = 0; j < n_pos; ++j) {
            tokens_out[j] = host[3 * j];
            std::memcpy(&logprobs_out[j], &host[3 * j + 1], 4);
        }
        const int* r4 = host.data() + n_pos * 3;
        result->accepted = r4[0];
        result->next_token = r4[1];
        std::memcpy(&result->next_logprob, &r4[2], 4);
        std::memcpy(&result->sum_logprob, &r4[3], 4);
        result->no_speech_prob = NAN;
        return WLK_OK;
    });
}

}  // extern "C"
