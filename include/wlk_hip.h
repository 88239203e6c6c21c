/*
 * wlk_hip.h - C ABI of libwlk_hip.so, the MI355X (gfx950) backend for WhisperLiveKit's
 * simul_whisper hot path.
 *
 * The reference has no FFI for this path: its plugin boundary is the set of abstract tensor
 * hooks of AlignAttBase (whisperlivekit/simul_whisper/align_att_base.py:541-649), implemented
 * in PyTorch by AlignAtt (whisperlivekit/simul_whisper/simul_whisper.py:108-462).  Each entry
 * point below names the hook(s)/reference code it replaces.  Everything is plain pointers and
 * sizes; `float*` arguments marked "host" are host memory, "dev" are device (HBM) pointers.
 *
 * Conventions
 *  - every function returns 0 (WLK_OK) or a negative error code; wlk_last_error() returns the
 *    message of the last failure on the calling thread (the Python shim raises RuntimeError,
 *    matching the reference's exception convention, simul_whisper/backend.py:266-268).
 *  - a wlk_model is immutable after wlk_model_finalize() and may be shared by any number of
 *    sessions / threads; a wlk_session is used by one thread at a time (the reference's
 *    threading contract).
 *  - all arithmetic is fp32 (whisper/model.py:39-50 keeps fp32 end to end on this path).
 */
#ifndef WLK_HIP_H
#define WLK_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WLK_OK 0
#define WLK_ERR_ARG (-1)
#define WLK_ERR_HIP (-2)
#define WLK_ERR_STATE (-3)
#define WLK_ERR_CAPACITY (-4)

typedef struct wlk_model wlk_model;
typedef struct wlk_session wlk_session;

/* ModelDimensions, whisperlivekit/whisper/model.py:26-37 */
typedef struct wlk_dims {
    int32_t n_mels, n_audio_ctx, n_audio_state, n_audio_head, n_audio_layer;
    int32_t n_vocab, n_text_ctx, n_text_state, n_text_head, n_text_layer;
} wlk_dims;

const char* wlk_last_error(void);
int wlk_abi_version(void);
/* number of visible HIP devices (0 if none / runtime unusable); never fails */
int wlk_device_count(void);

/* ---- weights: one packed fp32 arena per GPU ------------------------------------------------
 * Replaces load_model()'s `.to(device)` of an nn.Module (whisper/__init__.py:466-596): tensors
 * keep the reference checkpoint names; conv weights are stored tap-major and q/k/v (k/v for
 * cross attention) are stored concatenated so each projection is one GEMM - the repacking is
 * done by the host shim, the layout is defined by wlk_tensor_lookup(). */
int wlk_arena_floats(const wlk_dims* dims, uint64_t* n_floats);
int wlk_tensor_lookup(const wlk_dims* dims, const char* packed_name, uint64_t* offset_floats,
                      uint64_t* numel);
/* n-th packed tensor name (0 <= index < count); returns WLK_ERR_ARG past the end */
int wlk_tensor_name(const wlk_dims* dims, int index, const char** name);

/* arena_dev may be NULL (the library hipMallocs it) or a caller-owned device buffer of
 * wlk_arena_floats() floats (e.g. a torch tensor that torch.distributed broadcasts over RCCL) */
int wlk_model_create(const wlk_dims* dims, int device, float* arena_dev, wlk_model** out);
int wlk_model_arena(wlk_model* m, float** arena_dev, uint64_t* n_floats);
int wlk_model_upload(wlk_model* m, const char* packed_name, const float* host, uint64_t numel);
/* (decoder layer, head) pairs in alignment-rank order; Whisper.set_alignment_heads,
 * whisper/model.py:363-370 + simul_whisper.py:151-159 */
int wlk_model_set_alignment_heads(wlk_model* m, const int32_t* layer_head_pairs, int n_pairs);
int wlk_model_finalize(wlk_model* m);
int wlk_model_destroy(wlk_model* m);

/* ---- per-stream session --------------------------------------------------------------------
 * Owns what DecoderState owns (simul_whisper/decoder_state.py:7-91) that is tensor-valued:
 * the rolling audio buffer, KV caches, the 16-step cross-attention window, workspaces, and a
 * HIP stream. */
int wlk_session_create(wlk_model* m, int beam, int max_audio_samples, wlk_session** out);
int wlk_session_destroy(wlk_session* s);
/* 1 = keep pre-softmax cross-attention QK of every layer/head and raw logits for wlk_export */
int wlk_session_set_debug(wlk_session* s, int on);

/* a1: AlignAtt.insert_audio (simul_whisper.py:219-237): append a chunk / evict the oldest
 * samples / drop everything.  Only the new chunk crosses PCIe. */
int wlk_audio_append(wlk_session* s, const float* pcm_host, int n);
/* (f-next, rank 3) the same append for int16 PCM as it arrives on the wire: replaces convert_pcm_to_float
 * (whisperlivekit/audio_processor.py:416-418: int16 -> float32 / 32768.0) + the fp32 upload; half the PCIe bytes */
int wlk_audio_append_pcm16(wlk_session* s, const int16_t* pcm_host, int n);
int wlk_audio_append_zeros(wlk_session* s, int n);
int wlk_audio_drop_front(wlk_session* s, int n);
int wlk_audio_clear(wlk_session* s);
int wlk_audio_len(wlk_session* s, int* n);

/* a2+a3+a4: AlignAtt._encode (simul_whisper.py:344-352) = log_mel_spectrogram(padding=30 s)
 * -> first 3000 frames -> AudioEncoder.forward, plus the cross-attention K/V projection of
 * every decoder layer (MultiHeadAttention.forward's first-use branch, whisper/model.py:117-126).
 * content_mel_len = int((T_padded - 3000) / 2). */
int wlk_encode(wlk_session* s, int32_t* content_mel_len);

/* a5: TextDecoder.forward(tokens, xa, kv_cache, return_cross_attn=True) (whisper/model.py:279-332)
 * via AlignAtt._get_logits_and_cross_attn (simul_whisper.py:357-368).  tokens: host int64
 * [n_rows, n_tok] row-major, n_rows = beam.  first != 0 starts a new `infer` (empty self-attn
 * cache and alignment window, i.e. after DecoderState.clean_cache()).  Logits are produced for
 * the last position and, when first, for position sot_index (the only rows the policy reads,
 * align_att_base.py:226-229); softmaxed cross-attention rows of the alignment heads go to the
 * session's 16-step window (align_att_base.py:221-224). Asynchronous on the session stream. */
int wlk_decode(wlk_session* s, const int64_t* tokens, int n_rows, int n_tok, int first, int sot_index);

/* a6: AlignAtt._check_no_speech (simul_whisper.py:370-377): softmax(logits[:, sot_index])[token] */
int wlk_no_speech_prob(wlk_session* s, int no_speech_token, float* probs_host /* [n_rows] */);

/* f4 (batch `transcribe`): the per-step logit rules of whisper's DecodingTask and the greedy pick at temperature 0 for ONE
 * sequence, on the device - SuppressBlank / SuppressTokens / ApplyTimestampRules (whisper/decoding.py:417-499) and
 * GreedyDecoder.update (whisper/decoding.py:270-287).  wlk_rules_set uploads the two token lists of a DecodingTask
 * (decoding.py:609-636 `_get_suppress_tokens`, :424 blank = encode(" ") + [eot]); wlk_pick_greedy applies the rules to the
 * logits of the last wlk_decode and returns the chosen token and its log-probability (8 bytes instead of the logits row).
 * The host derives the history-dependent fields from the sampled tokens exactly as ApplyTimestampRules.apply does:
 *   ts_mode  0: the last sampled token is no timestamp; 1: the last two are timestamps (or only one token was sampled and
 *            it is one) - timestamps are suppressed; 2: only the last one is - text tokens below eot are suppressed
 *   ts_bound timestamps in [timestamp_begin, ts_bound) are suppressed (timestamp_begin = none)
 *   max_initial  first step only: timestamps above timestamp_begin + max_initial are suppressed (-1 = no limit) */
typedef struct wlk_pick_params {
    int32_t first_step, without_timestamps, timestamp_begin, eot, no_timestamps /* -1 = none */, ts_mode, ts_bound, max_initial;
} wlk_pick_params;
int wlk_rules_set(wlk_session* s, const int32_t* suppressed, int n_suppressed, const int32_t* blank, int n_blank);
int wlk_pick_greedy(wlk_session* s, const wlk_pick_params* p, int32_t* token_host, float* logprob_host);
/* The same rules for every row of a session with beam == n_rows (1..8), each row with its own parameter block - first_step,
 * without_timestamps and max_initial are the same in all; ts_mode and ts_bound follow each row's sampled tokens - and the
 * k (1..8) best log-probabilities of each row - what BeamSearchDecoder.update (whisper/decoding.py:332-338) reads, in one
 * read-back.  Applied to the logits of the last wlk_decode / wlk_decode_ancestry.  Entries are ordered by (log-probability
 * descending, id ascending); a row that allows fewer than k tokens fills up with (-inf, -1).  WLK_ERR_STATE before a decode
 * or before wlk_rules_set, WLK_ERR_ARG on a bad shape. */
int wlk_pick_topk(wlk_session* s, const wlk_pick_params* p /* [n_rows] */, int n_rows, int k,
                  float* logprobs_host /* [n_rows, k] */, int32_t* ids_host /* [n_rows, k] */);

/* Window groups (batch `transcribe`, opt-in): the greedy temperature-0 steps of up to 8 windows that belong to DIFFERENT
 * beam-1 sessions of one model as one launch chain - one pass over the decoder weights per token for all of them.  The
 * group owns a stream and the workspace of an 8-row step; sessions are not bound to it, any prefilled session of the
 * model may ride in any step.
 * wlk_group_step_pick: one single-token decoder step + logit rules + greedy pick for n (1..max_rows) distinct sessions.
 *   Row r feeds tokens[r] into sessions[r], applies that session's wlk_rules_set lists with p[r] and returns the token and
 *   log-probability wlk_pick_greedy would return (bit-identical for the same logits row).  Every session is checked on
 *   the host BEFORE anything is launched; a refused call has advanced no session: WLK_ERR_ARG for n outside 1..max_rows, a
 *   session listed twice, a session of another model or with beam != 1, a token or rule parameter out of range;
 *   WLK_ERR_STATE for a session before its prefill (the first wlk_decode of the window stays the session's own), before
 *   wlk_rules_set, with self_len + 1 > n_text_ctx, or attached to the batch engine (wlk_engine_attach: its single-token
 *   steps belong to the engine's loops).  The group's stream waits for what each session's stream has queued, the call
 *   returns after the read-back, and each session is left as its own wlk_decode of that token leaves it (position, KV
 *   cache, alignment window) - EXCEPT that the logits stay in the group: "logits_last" of wlk_export is not refreshed by
 *   a group step (wlk_group_export_logits reads them), so wlk_pick_greedy / wlk_select after a group step see the
 *   session's previous own decode.  A row's results do not depend on the rows beside it.  One step at a time per group;
 *   the caller keeps the sessions of a step to itself for its duration. */
typedef struct wlk_group wlk_group;
int wlk_group_create(wlk_model* m, int max_rows /* 1..8 */, wlk_group** out);
int wlk_group_destroy(wlk_group* g);   /* before the model */
int wlk_group_step_pick(wlk_group* g, wlk_session* const* sessions, const int64_t* tokens /* [n] */,
                        const wlk_pick_params* p /* [n] */, int n, int32_t* tokens_out /* [n] */, float* logprobs_out /* [n] */);
/* wlk_group_run_pick (opt-in): up to `burst` (1..16) such steps of every row behind ONE call - one upload, `burst`
 *   launch chains back to back with a one-wave kernel between them that derives each row's next step from its pick on the
 *   device (the next position and alignment-window row, the next ts_mode / ts_bound, first_step = 0), one read-back, one
 *   synchronisation.  Row r feeds tokens[r], then its own picks, for at most min(max_steps[r], burst, n_text_ctx - self_len)
 *   steps, and stops early after the step that picks p[r].eot.  steps_out[r] (>= 1) is the number of steps it took;
 *   tokens_out[r][0 .. steps - 1] and logprobs_out[r][0 .. steps - 1] are what that many successive wlk_group_step_pick calls
 *   return, bit for bit; entries at index >= steps are left as the caller passed them.  Afterwards every session is as
 *   after steps_out[r] single steps.  A row that has ended repeats its last step in the remaining chains, which rewrites
 *   the values already there.  The host checks are wlk_group_step_pick's, plus WLK_ERR_ARG for burst outside 1..16 and for
 *   a max_steps[r] < 1; a refused call has launched nothing and advanced nobody.  wlk_group_step_pick is the one-step
 *   case of the same routine. */
int wlk_group_run_pick(wlk_group* g, wlk_session* const* sessions, const int64_t* tokens /* [n] */,
                       const wlk_pick_params* p /* [n] */, const int32_t* max_steps /* [n], >= 1 */, int n, int burst /* 1..16 */,
                       int32_t* tokens_out /* [n][burst] */, float* logprobs_out /* [n][burst] */, int32_t* steps_out /* [n] */);
/* steps: launch chains enqueued; rows: row-steps actually taken (wlk_group_run_pick: chains x rows minus rows is what rows
 * that had ended took up) */
int wlk_group_stats(wlk_group* g, uint64_t* steps, uint64_t* rows);
/* tests: the logits row [n_vocab] of slot `row` of the last completed step (WLK_ERR_STATE: no such row) */
int wlk_group_export_logits(wlk_group* g, int row, float* host, uint64_t capacity, uint64_t* n_written);
/* Stacked word alignment (opt-in): what wlk_find_alignment computes for up to max_rows windows of DIFFERENT
 * encoded beam-1 sessions of the group's model in one call - ONE teacher-forced decoder pass over the rows of all windows
 * (the stacked prefill chain: a row goes through its session's own arithmetic), the token probabilities per window with the
 * solo call's launches, the attention normalisation, the warping recurrence (one workgroup per window, side by side) and the
 * path walk as six launches for all windows, and ONE read-back of about 1 KB per window.
 *   starts[i], i = 0 .. n_text: the frame index at which the warping path enters text row i (the last entry is the
 *     <|endoftext|> row) - time_indices[first element of text index i] of whisper/timing.py's backtrace, with its overrides
 *     (row 0 only moves left, column 0 only moves up); all that word_timings reads of the path.
 *   token_probs, cost, trace: as wlk_find_alignment returns them (cost and trace are optional and copied only where asked).
 * Every window is checked on the host BEFORE anything is launched or any session is touched: WLK_ERR_ARG for n outside
 * 1..max_rows, a session listed twice, of another model or with beam != 1, everything wlk_find_alignment refuses about the
 * tokens, and a shape outside the stacked chain (wlk_group_align_fits); WLK_ERR_STATE for a session that is not encoded,
 * attached to the batch engine, or in debug / profiling mode.  The group's stream waits for what each session's stream has
 * queued; the call returns after one synchronisation of the group's stream.  Afterwards every session needs a new prefill
 * (wlk_decode, first = 1), as after wlk_find_alignment.  A window's results do not depend on the windows beside it.
 * The first call allocates the group's stacked-pass workspace for 8 x 256 rows (about 11 n_text_state + 1056 n_text_head
 * floats per row: 0.12 GB for base, 0.29 GB for large) and a buffer for logits, normalised attention and traces that grows
 * on demand; a group that never aligns allocates neither.
 * wlk_group_align_fits: the shape conditions alone, a pure host function of (model, n_tokens, num_frames): 9 <= n_tokens <=
 * min(256, n_text_ctx), every decoder GEMM of that many rows on the k-wave kernel (needs n_text_state >= 256), the
 * cross-attention with key splits, 1 <= num_frames / 2 <= n_audio_ctx, and a model with alignment heads. */
typedef struct wlk_align_window {
    wlk_session* s;            /* encoded beam-1 session of the group's model, not attached to the batch engine */
    const int64_t* tokens;     /* [sot sequence (n_sot) | <|notimestamps|> | text tokens | <|endoftext|>] */
    int32_t n_tokens, n_sot, eot, num_frames;
    float qk_scale;
    int32_t* starts;           /* out [n_text + 1] */
    float* token_probs;        /* out [n_text] */
    float* cost;               /* optional out [n_text + 1][num_frames / 2] */
    int8_t* trace;             /* optional out (n_text + 2) x (num_frames / 2 + 1) */
} wlk_align_window;
int wlk_group_find_alignment(wlk_group* g, const wlk_align_window* w, int n /* 1..max_rows */);
int wlk_group_align_fits(wlk_group* g, int32_t n_tokens, int32_t num_frames, int32_t* fits);
/* Draft verification (opt-in): how much of a draft - the tokens the previous call of a growing buffer produced -
 * greedy decoding at temperature 0 would produce again, and the token behind it, for up to max_rows windows of DIFFERENT
 * encoded beam-1 sessions in one call: ONE teacher-forced decoder pass over [initial tokens | draft] of all windows (the
 * stacked prefill chain), per window the final LayerNorm and vocabulary projection of the n_draft + 1 candidate rows (row
 * n_initial - 1 + j predicts what follows draft[0 .. j)) and of the sot row, the greedy pick of every candidate row under the
 * rule state its position has (derived on the device from p, the state of the window's FIRST pick, and the draft), and
 *   accepted k   = the first j with pick(j) != draft[j] (n_draft when there is none),
 *   next_token, next_logprob = the pick at position k (the bits wlk_pick_greedy gives on that logits row),
 *   sum_logprob  = the log-probabilities of positions 0 .. k added in ascending order in fp32 (nothing is added, and
 *                  next_token is p.eot, when tokens[n_initial - 1] is p.eot already),
 *   no_speech_prob = softmax(logits of row sot_index)[no_speech_token] (NaN for no_speech_token < 0).
 * Afterwards every session is what its own prefill of [initial | draft[0 .. k)] leaves - position n_initial + k, its K/V rows
 * below that, wlk_no_speech_prob, wlk_pick_greedy and wlk_export("logits_last") included (the logits row of position k) -
 * and the caller goes on by feeding next_token (wlk_decode first = 0, wlk_group_step_pick, wlk_group_run_pick).  K/V rows at
 * and behind n_initial + k hold the rejected draft; every step overwrites its own position before anything reads it.
 * Every window is checked on the host BEFORE anything is launched or any session is touched: WLK_ERR_ARG for n outside
 * 1..max_rows, a session listed twice, of another model or with beam != 1, n_initial < 1, an empty draft, a draft token equal
 * to p.eot, a token or rule parameter out of range, sot_index outside the initial tokens, n_tokens > n_text_ctx or outside the
 * stacked chain's shapes (wlk_group_verify_fits), a score window shorter than n_tokens rows; WLK_ERR_STATE for a session that is
 * not encoded, has no wlk_rules_set lists, is attached to the batch engine or in debug / profiling mode.  A window's results do
 * not depend on the windows beside it.  The pass shares wlk_group_find_alignment's stacked workspace (allocated by the first
 * call of either) and a logits buffer of (longest draft + 2) x n_vocab floats that grows on demand.
 * wlk_group_verify_fits: the shape conditions alone, a pure host function of (model, n_initial, n_draft): n_initial >= 1,
 * n_draft >= 1, 9 <= n_initial + n_draft <= min(256, n_text_ctx), the decoder GEMMs of that many rows on the k-wave kernel,
 * the cross-attention with key splits. */
typedef struct wlk_verify_result {
    int32_t accepted, next_token;
    float next_logprob, sum_logprob, no_speech_prob;
} wlk_verify_result;
typedef struct wlk_verify_window {
    wlk_session* s;            /* encoded beam-1 session of the group's model with wlk_rules_set lists */
    const int64_t* tokens;     /* [initial tokens (n_initial) | draft (n_tokens - n_initial)] */
    int32_t n_initial, n_tokens, sot_index, no_speech_token /* -1 = none */;
    wlk_pick_params p;         /* the rule state of the window's first pick (position 0) */
    wlk_verify_result* result; /* out */
    int32_t* picks;            /* optional out (tests) [n_draft + 1][2]: token and log-probability bits of every position */
} wlk_verify_window;
int wlk_group_verify(wlk_group* g, const wlk_verify_window* w, int n /* 1..max_rows */);
int wlk_group_verify_fits(wlk_group* g, int32_t n_initial, int32_t n_draft, int32_t* fits);
/* Diagnostic (tests): the two kernels behind wlk_group_verify's decoder pass alone on host data - logits [n_draft + 1][n_vocab],
 * one rule mask [n_vocab] (as wlk_rules_set builds it), p0 = the first position's state, `ended` != 0: the token in front of
 * position 0 is <|endoftext|>.  tokens_out / logprobs_out [n_draft + 1]: every position's pick; result: accepted, next_token,
 * next_logprob, sum_logprob.  n_draft in 1..256.  Runs on the current device; needs no model.  Synchronous. */
int wlk_diag_draft_pick(const float* logits_host, int n_vocab, const uint8_t* mask_host, const wlk_pick_params* p0,
                        const int32_t* draft, int n_draft, int ended, int32_t* tokens_out, float* logprobs_out,
                        wlk_verify_result* result);
/* Diagnostic (tests): the ragged warping launches of wlk_group_find_alignment (recurrence, transposition, path walk) on n
 * (1..8) host cost matrices; matrix i is [n_rows[i]][n_cols[i]] at costs + offsets[i] (1..1024 rows, 1..4095 columns).
 * starts: n_rows[i] entries per matrix, concatenated; traces (optional): (n_rows[i] + 1) x (n_cols[i] + 1) step codes per
 * matrix, concatenated.  Runs on the current device; needs no model.  Synchronous. */
int wlk_diag_dtw_starts(const float* costs, const int64_t* offsets, const int32_t* n_rows, const int32_t* n_cols, int n,
                        int32_t* starts, int8_t* traces);
/* Diagnostic (tests): the rows pick kernel alone on host data - logits [n][n_vocab], n_masks (1..8) rule masks
 * [n_masks][n_vocab] (bit 0 = always suppressed, bit 1 = blank, as wlk_rules_set builds them), row r under
 * masks[mask_of_row[r]] and p[r]; n in 1..8.  Synchronous. */
int wlk_diag_pick_rows(const float* logits_host, int n_vocab, const uint8_t* masks_host, int n_masks, const int32_t* mask_of_row,
                       const wlk_pick_params* p /* [n] */, int n, int32_t* tokens_out, float* logprobs_out);
/* Diagnostic (tests): the one-row pick kernel behind wlk_pick_greedy alone on host data - one logits row [n_vocab], one rule
 * mask [n_vocab] and one parameter block; token_out [1], logprob_bits_out [1] = the bits of the log-probability.  And the
 * top-k kernel behind wlk_pick_topk: logits [n_rows][n_vocab] (n_rows in 1..8), one rule mask, p [n_rows], k in 1..8;
 * logprobs_out / ids_out [n_rows][k], ordered and filled up as wlk_pick_topk's.  WLK_ERR_ARG, before anything is uploaded,
 * for a NULL pointer, a count out of range or a parameter block wlk_group_step_pick would refuse.  On the device the logits
 * and the masks of these two entries, of wlk_diag_pick_rows and of wlk_diag_draft_pick are followed by one guard entry (+inf,
 * allowed): a kernel that reads past the last row returns token n_vocab.
 * Run on the current device; need no model.  Synchronous. */
int wlk_diag_pick_one(const float* logits_host, int n_vocab, const uint8_t* mask_host, const wlk_pick_params* p, int32_t* token_out,
                      uint32_t* logprob_bits_out);
int wlk_diag_pick_topk(const float* logits_host, int n_vocab, const uint8_t* mask_host, const wlk_pick_params* p /* [n_rows] */,
                       int n_rows, int k, float* logprobs_out /* [n_rows][k] */, int32_t* ids_out /* [n_rows][k] */);
/* Diagnostic (tests): the device form of the rule transition of wlk_group_run_pick alone - out[i] = the parameter block of
 * the step after tokens[i] was picked under p[i].  Needs no model; any n >= 1.  Synchronous. */
int wlk_diag_pick_advance(const wlk_pick_params* p /* [n] */, const int32_t* tokens /* [n] */, int n, wlk_pick_params* out /* [n] */);

/* a6+a7+a8 in one launch group and ONE readback:
 *  - logits[row, ids[i]] += deltas[i] (-inf suppresses: SuppressTokens.apply whisper/decoding.py:427-432,
 *    _suppress_blank_tokens simul_whisper.py:379-381, DRY penalty align_att_base.py:492-537);
 *  - log_softmax + top-k (the device part of BeamSearchDecoder.update, whisper/decoding.py:332-338);
 *  - AlignAtt._process_cross_attention + _get_attended_frames (simul_whisper.py:390-437) over the
 *    current window: most attended frame of the newest row, per beam row.
 * adj_row[i] < 0 applies the adjustment to every row. */
int wlk_select(wlk_session* s, const int32_t* adj_row, const int32_t* adj_ids, const float* adj_deltas,
               int n_adj, int k, int content_mel_len,
               float* top_logprobs_host /* [n_rows, k] */, int32_t* top_ids_host /* [n_rows, k] */,
               int32_t* frames_host /* [n_rows] */);

/* BeamPyTorchInference.rearrange_kv_cache (simul_whisper/beam.py:15-19) */
int wlk_kv_reorder(wlk_session* s, const int32_t* source_rows, int n_rows);

int wlk_sync(wlk_session* s);

/* ---- (f-next, rank 1) the AlignAtt decode loop of one infer behind ONE call -------------------------------
 * Replaces the per-token Python loop of AlignAttBase.infer (simul_whisper/align_att_base.py:206-286) for beam 1:
 * decoder forward, no-speech check (first step), blank / special-token suppression, DRY penalty
 * (align_att_base.py:492-537), BeamSearchDecoder.update with beam_size 1 (whisper/decoding.py:317-376), AlignAtt
 * read-out and the stop rules (completed / rewind / frame threshold / token budget) - no Python between tokens.
 * The caller keeps everything before and after the loop (context trimming, word splitting, timestamps). */
typedef struct wlk_loop_params {
    int32_t sot_index;            /* index of <|startoftranscript|> in the fed tokens (no-speech row) */
    int32_t is_last;
    int32_t frame_threshold;      /* cfg.frame_threshold (4 is used when is_last) */
    int32_t rewind_threshold;     /* cfg.rewind_threshold */
    int32_t last_attend_frame;    /* state.last_attend_frame on entry */
    int32_t max_text_len;         /* model.dims.n_text_ctx */
    int32_t budget;               /* max(50, int(seconds * 15 * 1.5)): decoder forwards allowed in this infer */
    int32_t eot;                  /* tokenizer.eot */
    int32_t dec_pad;              /* DEC_PAD = 50257 (align_att_base.py:9) */
    int32_t no_speech_token;      /* < 0: no check */
    float no_speech_threshold;    /* cfg.nonspeech_prob */
    int32_t content_mel_len;      /* from wlk_encode, unclipped */
    /* Teacher forcing of single decisions, for parity harnesses only (0 entries in production): when a decision of
     * this library and the reference's differ inside an fp32 tie (two candidates closer than rounding), the harness
     * replays the stream with the reference's choice forced at that step so that every later decision can still be
     * compared.  Entry f applies to decode step force_step[f] of this loop (0 = the prefill's read-out): the attended
     * frame becomes force_frame[f] (if >= 0); the selected token becomes force_token[f] (if >= 0) provided it is the
     * runner-up of the step's top-2 and the winner is not end-of-text (the two are then swapped, log-probs included). */
    int32_t n_force;              /* 0 .. WLK_MAX_FORCED */
    int32_t force_step[4];
    int32_t force_token[4];
    int32_t force_frame[4];
} wlk_loop_params;
#define WLK_MAX_FORCED 4
enum {
    WLK_STOP_NONE = 0,
    WLK_STOP_CONTEXT_FULL = 1,    /* tokens reached max_text_len */
    WLK_STOP_BUDGET = 2,          /* runaway guard: every token of this infer is dropped */
    WLK_STOP_NO_SPEECH = 3,
    WLK_STOP_COMPLETED = 4,       /* end-of-text won: the last appended token is dropped */
    WLK_STOP_REWIND = 5,          /* attention jumped back: every token of this infer is dropped */
    WLK_STOP_FRAME = 6            /* attention reached the end of the audio: the last appended token is dropped */
};
typedef struct wlk_loop_result {
    int32_t n_steps;              /* decode steps that selected a token (= entries of step_tokens / step_frames) */
    int32_t n_new_tokens;         /* tokens kept (after the drops above) */
    int32_t stop_reason;
    int32_t last_attend_frame;    /* state.last_attend_frame on exit */
    float no_speech_prob;
    float sum_logprob;
    int32_t decode_calls;         /* decoder forwards run */
} wlk_loop_result;
/* tokens: host int64 [n_tok] = context + prompt (what _current_tokens() returns, one row).  suppress_ids: the
 * SuppressTokens list; blank_ids: encode(" ") + [eot].  Outputs (each of capacity `cap`, may be NULL except result):
 * the kept new tokens, and per decode step the selected token, the attended frame and the running log-prob sum.
 * The session must have been encoded; its beam must be 1.  Sessions attached to a batch engine (wlk_engine_attach)
 * run their single-token steps batched with the other attached sessions of the model. */
int wlk_decode_until_stop(wlk_session* s, const int64_t* tokens, int n_tok, const wlk_loop_params* p,
                          const int32_t* suppress_ids, int n_suppress, const int32_t* blank_ids, int n_blank,
                          wlk_loop_result* result, int64_t* new_tokens, int32_t* step_tokens, int32_t* step_frames,
                          float* step_sum_logprobs, int cap);
/* Cross-session batching of those loops: the reference serves N sessions from one model on one device
 * (whisperlivekit/core.py:246-271, audio_processor.py:543-551), each issuing its own launch chain per token.  Sessions
 * attached here hand the single-token steps of wlk_decode_until_stop to ONE worker per GPU that advances every loop
 * currently in its decode phase in one launch chain (rows = sessions; weights are streamed once per step for all of
 * them; per-row arithmetic and its order are those of a session running alone).  The prefills (first decoder pass of an
 * infer) that are waiting at the same time run as one stacked chain as well (csrc/api.hip: wlk_prefill_group), bit-identical
 * to a session's own prefill.  Beam-1 sessions only. */
int wlk_engine_attach(wlk_session* s);
int wlk_engine_detach(wlk_session* s);
/* encode launch chains run by the engine and the sessions encoded in them (concurrent wlk_encode calls of attached
 * sessions are stacked: one launch per encoder operator with grid.y = sessions, shared weights) */
int wlk_engine_encode_stats(wlk_model* m, uint64_t* batches, uint64_t* sessions);
/* engine iterations, rows advanced in them, and the batched (>= 2 rows) iterations / rows among those */
int wlk_engine_stats(wlk_model* m, uint64_t* iterations, uint64_t* rows, uint64_t* batched_steps, uint64_t* batched_rows);
/* The host half of that loop without a GPU (integer logic only), for harnesses that supply the numerics themselves:
 * begin_step -> n_feed tokens to run through the decoder (0 = loop over); no_speech (first step only); adjustments ->
 * unique (id, additive delta) pairs to apply to the last-position logits; consume(top-2 log-probs/ids after the
 * adjustments, attended frame) -> goes_on. */
typedef struct wlk_decode_job wlk_decode_job;
int wlk_job_create(const wlk_loop_params* p, const int64_t* tokens, int n_tok, const int32_t* suppress_ids, int n_suppress,
                   const int32_t* blank_ids, int n_blank, wlk_decode_job** out);
int wlk_job_begin_step(wlk_decode_job* j, int32_t* n_feed);
int wlk_job_no_speech(wlk_decode_job* j, float prob, int32_t* stops);
int wlk_job_adjustments(wlk_decode_job* j, const int32_t** ids, const float** deltas, int32_t* n);
int wlk_job_consume(wlk_decode_job* j, const float* top_logprobs, const int32_t* top_ids, int frame, int32_t* goes_on);
int wlk_job_result(wlk_decode_job* j, wlk_loop_result* result, int64_t* new_tokens, int32_t* step_tokens,
                   int32_t* step_frames, float* step_sum_logprobs, int cap);
int wlk_job_destroy(wlk_decode_job* j);

/* ---- the same loop for the beam decoder, beams 2..7 ----------------------------------------------------------------
 * wlk_decode_beam_until_stop: arguments as wlk_decode_until_stop; `tokens` is the prompt of ONE row (the prefill feeds
 * beam copies of it, as AlignAttBase does).  Per step: decoder forward over the beam rows, the adjustments (computed from
 * row 0, applied to every row), top-(beam+1) per row + the AlignAtt read-out in one read-back, BeamSearchDecoder.update
 * (whisper/decoding.py:317-376, patience 1) and the stop rules on row 0.  The result describes row 0 (step_sum_logprobs:
 * sum_logprobs[0] after each update).  No teacher forcing (n_force must be 0).
 * Single-token steps do not copy the self-attention cache when the hypotheses are re-ranked: a device table
 * anc[beam][n_text_ctx] names, per hypothesis and position, the physical cache row that holds it, and the step's
 * self-attention reads through it.  Once such a step has run in an infer the physical rows no longer are the
 * hypotheses, so wlk_decode(first = 0) and wlk_kv_reorder on that session return WLK_ERR_STATE until the next
 * wlk_decode(first = 1).  Debug / profiling sessions and shapes the <= 8-row weight-streaming kernels do not take
 * run every step as wlk_decode + wlk_select + wlk_kv_reorder inside this call instead. */
int wlk_decode_beam_until_stop(wlk_session* s, const int64_t* tokens, int n_tok, const wlk_loop_params* p,
                               const int32_t* suppress_ids, int n_suppress, const int32_t* blank_ids, int n_blank,
                               wlk_loop_result* result, int64_t* new_tokens, int32_t* step_tokens, int32_t* step_frames,
                               float* step_sum_logprobs, int cap);
/* One single-token step of a beam session whose row b continues hypothesis source_rows[b] of the previous step: what
 * wlk_kv_reorder(source_rows) followed by wlk_decode(first = 0) computes.  Sessions that qualify (see above) take the step
 * over the ancestry table, nothing moves in the cache, and the rule above holds: wlk_decode(first = 0) and wlk_kv_reorder
 * are refused until the next wlk_decode(first = 1).  Every other session makes those two calls inside this one.  Which of
 * the two a session takes does not change during an infer. */
int wlk_decode_ancestry(wlk_session* s, const int64_t* tokens /* [n_rows] */, const int32_t* source_rows, int n_rows);
/* single-token steps of this session that ran over the ancestry table so far (either entry point) */
int wlk_session_beam_stats(wlk_session* s, uint64_t* ancestry_steps);
/* Diagnostic (tests): one single-token decoder forward over the ancestry table - what wlk_decode(first = 0) computes
 * after wlk_kv_reorder(source_rows), without moving the cache.  WLK_ERR_STATE when the session does not qualify. */
int wlk_diag_beam_step(wlk_session* s, const int64_t* tokens, const int32_t* source_rows, int n_rows);
/* Host half of the beam loop without a GPU, as wlk_job_*: consume takes the [beam][beam + 1] log-probs / ids after the
 * adjustments and the [beam] attended frames; state hands back the hypotheses ([beam][row_len], rank order), their
 * sum_logprobs, the source row of each in the last update and whether `finished` is full. */
typedef struct wlk_beam_job wlk_beam_job;
int wlk_beam_job_create(const wlk_loop_params* p, int beam, const int64_t* tokens, int n_tok, const int32_t* suppress_ids,
                        int n_suppress, const int32_t* blank_ids, int n_blank, wlk_beam_job** out);
int wlk_beam_job_begin_step(wlk_beam_job* j, int32_t* n_feed);
int wlk_beam_job_no_speech(wlk_beam_job* j, float prob, int32_t* stops);
int wlk_beam_job_adjustments(wlk_beam_job* j, const int32_t** ids, const float** deltas, int32_t* n);
int wlk_beam_job_consume(wlk_beam_job* j, const float* top_logprobs, const int32_t* top_ids, const int32_t* frames,
                         int32_t* goes_on);
int wlk_beam_job_state(wlk_beam_job* j, int64_t* rows, int cap, int32_t* row_len, float* sum_logprobs, int32_t* source_rows,
                       int32_t* completed);
int wlk_beam_job_result(wlk_beam_job* j, wlk_loop_result* result, int64_t* new_tokens, int32_t* step_tokens,
                        int32_t* step_frames, float* step_sum_logprobs, int cap);
int wlk_beam_job_destroy(wlk_beam_job* j);

/* ---- CIF end-of-word head on the device (opt-in) -------------------------------------------------------
 * Replaces, for callers that ask for it, the host evaluation of simul_whisper/eow_detection.py:62-77 (fire_at_boundary) and
 * the read-back of the encoder output it needs.  The head (a Linear(n_audio_state, 1): weight [d] and bias) lives in a
 * device buffer of the model beside the weight arena; weight_host == NULL removes it.  d != n_audio_state: WLK_ERR_ARG.
 * While a model has a head, every wlk_encode enqueues two small kernels behind the cross-attention K/V projection, on
 * the stream the encode runs on: alpha[t] = sigmoid(x[t] . w + b) over the T = min(content_mel_len, n_audio_ctx) content
 * rows, then resize() and the integrate-and-fire test in fp32, leaving the record below in host-coherent memory.  Models
 * without a head launch and allocate nothing.  Not to be called while an encode of the model is in flight. */
typedef struct wlk_cif_out {
    int32_t fire;            /* the decision: 1 = the chunk ends at a word boundary */
    int32_t n;               /* round(sum(alpha)), ties to even */
    int32_t cnt;             /* floor(integrate[-1] / 0.999) */
    int32_t pos;             /* first index with integrate - cnt >= 0, -1 = none */
    int32_t resize_rounds;   /* rounds of resize()'s loop that ran (0..10) */
    float total;             /* sum(alpha) */
    float integ_last;        /* integrate[-1] = cumsum(alpha')[T - 2] */
    uint32_t seq;            /* sequence number of the encode the record belongs to; written last */
} wlk_cif_out;
int wlk_model_set_cif(wlk_model* m, const float* weight_host, int d, float bias);
/* The record of the session's last encode.  WLK_ERR_STATE when the model has no head, nothing has been encoded with it,
 * or that encode had fewer than two content frames (the reference raises there).  Waits for the encode's stream only if
 * the record has not arrived yet. */
int wlk_cif_result(wlk_session* s, wlk_cif_out* out);
/* Diagnostic (tests): the two production kernels on host data.  feat_host holds n_stack (1..8) blocks of [T][d]; block i
 * is evaluated over its first t_each[i] rows (t_each == NULL: T rows each) as session i of one stacked launch, from fp32
 * rows or, as_x3 != 0, from the X3 image packed on the device.  alphas_out [n_stack][T] (may be NULL), out [n_stack]. */
int wlk_diag_cif(const float* feat_host, int T, int d, const float* weight, float bias, int as_x3, int n_stack,
                 const int32_t* t_each, float* alphas_out, wlk_cif_out* out);

/* Parity/debug exports to host memory.  what: "mel" [n_mels,3000], "enc" [1500,d],
 * "logits_last" / "logits_sot" [n_rows,V], "attn_last" [n_rows, content_mel_len] (after
 * wlk_select), "cross_qk:<layer>" [rows, H, 1500] of the latest wlk_decode (debug sessions only),
 * "self_k:<layer>" [n_rows, len, d], "xattn_w:<rank>" [window rows, 1500]. */
int wlk_export(wlk_session* s, const char* what, float* host, uint64_t capacity, uint64_t* n_written);

/* Per-kernel timing of the session's stream with HIP events (bench.py roofline leg).
 * wlk_prof_begin arms it; wlk_prof_end fills, per launch tag (up to cap entries): summed event
 * time in ms, launch count, and the summed ALGORITHMIC flops / bytes of those launches. */
int wlk_prof_begin(wlk_session* s);
int wlk_prof_end(wlk_session* s, int cap, const char** names, float* total_ms, int32_t* launches,
                 double* flops, double* bytes, int32_t* n_out);

/* Wall time of the session's single-token decode steps so far (graph-replayed steps of wlk_decode_until_stop outside
 * the batch engine): number of steps, nanoseconds from entering the step to holding its result (graph launch + the 46
 * kernels + the flag wait), and the share of that spent inside hipGraphLaunch.  What bench.py's roofline.step divides the
 * step's algorithmic bytes by. */
int wlk_session_step_stats(wlk_session* s, uint64_t* steps, uint64_t* wall_ns, uint64_t* launch_ns);

/* ---- a12 front end: log-mel features of the streaming Sortformer diarizer ----------------------
 * Replaces NeMo's AudioToMelSpectrogramPreprocessor.get_features as called at
 * whisperlivekit/diarization/sortformer_backend.py:181-188,273-275 (window 25 ms, stride 10 ms, n_fft 512,
 * 128 mel bins, normalize "NA", pre-emphasis 0.97, log(x + 2^-24)).  filters: [n_mels, n_fft/2+1];
 * window: [win_length] (symmetric hann).  Output is time-major [n_frames, n_mels], n_frames = n/hop + 1. */
typedef struct wlk_melspec wlk_melspec;
int wlk_melspec_create(int device, int n_fft, int win_length, int hop, int n_mels, const float* filters,
                       const float* window, float preemph, float log_guard, int max_samples, wlk_melspec** out);
int wlk_melspec_run(wlk_melspec* m, const float* pcm_host, int n, float* out_host, int capacity_frames,
                    int* n_frames);
int wlk_melspec_destroy(wlk_melspec* m);

/* ---- a12 network: the streaming Sortformer diarizer ------------------------------------------------
 * Replaces what the reference gets from NeMo's SortformerEncLabelModel at
 * whisperlivekit/diarization/sortformer_backend.py:108-131 (load, streaming configuration) and :293-300
 * (forward_streaming_step): ConvSubsampling(dw_striding, x8) -> 17 Conformer blocks (relative-position
 * attention) -> Linear -> 18 post-LN Transformer blocks -> sigmoid speaker head.  NeMo is a third-party
 * dependency that is not in the reference tree: packed tensor names/layout are defined by wlk_sf_tensor_name /
 * wlk_sf_tensor_lookup, the host shim (whisperlivekit_amd/sortformer.py) maps NeMo state-dict names onto them.
 * The streaming speaker-cache / FIFO bookkeeping (SortformerModules.streaming_update_async) is host logic, unless the
 * session is device-resident (wlk_sf_session_*, below). */
typedef struct wlk_sortformer wlk_sortformer;
typedef struct wlk_sf_dims {
    int32_t n_mels;        /* 128 */
    int32_t sub_channels;  /* 256: conv channels of the sub-sampling stem */
    int32_t fc_d_model, fc_layers, fc_heads, fc_ff, conv_kernel;   /* 512, 17, 8, 2048, 9 */
    int32_t tf_d_model, tf_layers, tf_heads, tf_inner;             /* 192, 18, 8, 768 */
    int32_t n_spk;         /* 4 */
    int32_t max_frames;    /* longest [spkcache | fifo | chunk] sequence, <= 512 */
    int32_t max_feat_frames; /* longest feature chunk handed to wlk_sf_step */
    float xscale;          /* sqrt(fc_d_model) when the encoder was trained with xscaling, else 1 */
} wlk_sf_dims;
int wlk_sf_arena_floats(const wlk_sf_dims* dims, uint64_t* n_floats);
int wlk_sf_tensor_lookup(const wlk_sf_dims* dims, const char* packed_name, uint64_t* offset_floats, uint64_t* numel);
int wlk_sf_tensor_name(const wlk_sf_dims* dims, int index, const char** name);
int wlk_sf_create(const wlk_sf_dims* dims, int device, wlk_sortformer** out);
int wlk_sf_upload(wlk_sortformer* m, const char* packed_name, const float* host, uint64_t numel);
/* precomputes linear_pos(pos_emb) of every Conformer block for max_frames (input independent) */
int wlk_sf_finalize(wlk_sortformer* m);
/* One streaming step (the device part of forward_streaming_step): feats_host [n_feat, n_mels] time-major log-mel
 * -> pre_encode -> chunk embeddings [n_chunk, fc_d_model] (returned in chunk_embs_host, n_chunk in *n_chunk);
 * ctx_embs_host [n_ctx, fc_d_model] = the caller's valid speaker-cache rows followed by its valid FIFO rows;
 * the network runs over [ctx | chunk] and preds_host receives [n_ctx + n_chunk, n_spk] sigmoid activities.
 * n_feat == 0 runs the network over ctx only; n_ctx == 0 over the chunk only.  Thread-safe; sessions keep their state on
 * the host.  Calls of several threads that wait for the model at the same time run as ONE stacked launch chain (their rows
 * one after the other, up to 8 sessions); a session's outputs are bit for bit those of its step alone. */
int wlk_sf_step(wlk_sortformer* m, const float* feats_host, int n_feat, const float* ctx_embs_host, int n_ctx,
                float* chunk_embs_host, int chunk_capacity_rows, int* n_chunk, float* preds_host,
                int preds_capacity_rows);
/* The same step with its front end inside (what sortformer_backend.py:273-300 does in three calls): pcm_host [n_pcm] is the new
 * audio chunk; its log-mel rows (n_pcm / hop + 1 of them, rows from valid_frames on zeroed - FilterbankFeatures' seq_len rule -
 * unless valid_frames < 0) are computed by `mel`'s kernel on the step's own stream, placed behind prev_feats_host [n_prev, n_mels]
 * (the rows the caller kept from its previous chunk, :279-283) and handed to the stem; feats_out_host receives the new rows
 * (*n_feats_out of them) so the caller can keep them for its next chunk.  Bit-identical to wlk_melspec_run + wlk_sf_step. */
int wlk_sf_step_pcm(wlk_sortformer* m, wlk_melspec* mel, const float* pcm_host, int n_pcm, int valid_frames,
                    const float* prev_feats_host, int n_prev, float* feats_out_host, int feats_capacity_rows, int* n_feats_out,
                    const float* ctx_embs_host, int n_ctx, float* chunk_embs_host, int chunk_capacity_rows, int* n_chunk,
                    float* preds_host, int preds_capacity_rows);
/* stacked launch chains run so far, the session steps inside them, their rows (batching statistics of the benchmark) */
int wlk_sf_stats(wlk_sortformer* m, uint64_t* stacked_steps, uint64_t* session_steps, uint64_t* rows);
/* parity/debug export of the last step (its first session): "fc_out" [T, fc_d_model] (Conformer output), "tf_out" [T, tf_d_model] */
int wlk_sf_export(wlk_sortformer* m, const char* what, float* host, uint64_t capacity, uint64_t* n_written);
/* WLK_ERR_STATE (and nothing freed) while sessions of the model are alive */
int wlk_sf_destroy(wlk_sortformer* m);

/* Device-resident diarizer sessions (opt-in): the streaming state of forward_streaming_step - speaker cache, FIFO, their
 * activities, the silence profile, the three lengths - and the last keep_feat_rows log-mel rows of the previous chunk live in
 * device buffers of the session.  A step runs the front end, the network over [spkcache | fifo | chunk] read from those buffers
 * and the state update (SortformerModules.streaming_update_async / _compress_spkcache, fp32 op for op as the numpy restatement
 * in whisperlivekit_amd/sortformer.py) in one launch chain; only the chunk's activities come back.  Session steps stack with
 * host-state steps (wlk_sf_step*) of the same model.  A session is used by one thread at a time: a call while another call of
 * the same session is in flight returns WLK_ERR_STATE. */
typedef struct wlk_sf_session wlk_sf_session;
typedef struct wlk_sf_cache_params {   /* SpkCacheParams (sortformer.py) */
    int32_t spkcache_len, fifo_len, spkcache_update_period, subsampling_factor, spkcache_sil_frames_per_spk;
    float pred_score_threshold, scores_boost_latest, sil_threshold, strong_boost_rate, weak_boost_rate, min_pos_scores_rate;
    int32_t max_index;
} wlk_sf_cache_params;
/* host view of a session's state: full buffers (spkcache [spkcache_len][d], spkcache_preds [spkcache_len][n_spk], fifo
 * [fifo_len][d], fifo_preds [fifo_len][n_spk], mean_sil_emb [d], kept_feats [keep_feat_rows][n_mels]) plus the lengths */
typedef struct wlk_sf_state {
    float *spkcache, *spkcache_preds, *fifo, *fifo_preds, *mean_sil_emb, *kept_feats;
    int32_t spkcache_len, fifo_len, n_sil_frames, n_kept;
} wlk_sf_state;
/* everything zeroed (new_state()); WLK_ERR_CAPACITY when the geometry does not fit the state kernels */
int wlk_sf_session_create(wlk_sortformer* m, const wlk_sf_cache_params* params, int keep_feat_rows, wlk_sf_session** out);
int wlk_sf_session_destroy(wlk_sf_session* s);
/* forward_streaming_step with the front end inside: pcm [n_pcm] -> log-mel rows behind the session's kept rows -> network ->
 * state update; chunk_preds_out receives the chunk's [*n_out][n_spk] activities; the chunk's last keep_feat_rows feature rows
 * become the kept rows.  left/right offsets in feature frames (converted with subsampling_factor like the host path). */
int wlk_sf_session_step_pcm(wlk_sf_session* s, wlk_melspec* mel, const float* pcm_host, int n_pcm, int valid_frames,
                            int left_offset, int right_offset, float* chunk_preds_out, int capacity_rows, int* n_out);
/* the same with the caller's feature rows [n_feat][n_mels] (forward_streaming_step); the kept rows are left as they are */
int wlk_sf_session_step(wlk_sf_session* s, const float* feats_host, int n_feat, int left_offset, int right_offset,
                        float* chunk_preds_out, int capacity_rows, int* n_out);
/* the state update alone on host-supplied chunk embeddings [Tc][d] and activities [T][n_spk] (T = spkcache_len + fifo_len
 * + Tc); lc / rc in embedding rows (streaming_update's arguments) */
int wlk_sf_session_update(wlk_sf_session* s, const float* chunk_embs, int Tc, const float* preds, int T, int lc, int rc,
                          float* chunk_preds_out, int capacity_rows, int* n_out);
int wlk_sf_session_get_state(wlk_sf_session* s, wlk_sf_state* st);
int wlk_sf_session_set_state(wlk_sf_session* s, const wlk_sf_state* st);

/* ---- (f-next, rank 3) Silero VAD gate -------------------------------------------------------------------
 * Replaces the TorchScript model the reference evaluates on the CPU once per 512-sample window
 * (whisperlivekit/silero_vad_iterator.py:163-184 load_jit_vad; called at :254 from VADIterator.__call__, driven by
 * FixedVADIterator :288-319 from audio_processor.py:1189-1190).  16 kHz model only.  The packed weight layout is
 * defined by wlk_vad_tensor_name / wlk_vad_tensor_lookup (the host shim transposes the archive's tensors).
 * A wlk_vad holds the weights of one GPU; a wlk_vad_stream holds what the TorchScript wrapper keeps per stream:
 * the 64-sample context and the LSTM (h, c).  wlk_vad_stream_run consumes n_windows x 512 samples and returns one
 * speech probability per window (two launches whatever n_windows is). */
typedef struct wlk_vad wlk_vad;
typedef struct wlk_vad_stream wlk_vad_stream;
int wlk_vad_weights_floats(uint64_t* n_floats);
int wlk_vad_tensor_lookup(const char* packed_name, uint64_t* offset_floats, uint64_t* numel);
int wlk_vad_tensor_name(int index, const char** name);
int wlk_vad_create(int device, const float* packed_host, uint64_t n_floats, wlk_vad** out);
int wlk_vad_destroy(wlk_vad* m);
int wlk_vad_stream_create(wlk_vad* m, int max_windows, wlk_vad_stream** out);
int wlk_vad_stream_reset(wlk_vad_stream* s);                       /* model.reset_states() */
int wlk_vad_stream_run(wlk_vad_stream* s, const float* pcm_host, int n_windows, float* probs_host);
int wlk_vad_stream_state(wlk_vad_stream* s, float* h_host /* [128] */, float* c_host /* [128] */);
int wlk_vad_stream_destroy(wlk_vad_stream* s);
/* wlk_vad_stream_run on int16 PCM as it comes off the wire: the samples are widened on the GPU as
 * (float)v * (1.0f / 32768.0f), the exact value of astype(float32) / 32768, so the result has the bits of
 * wlk_vad_stream_run on that fp32 audio. */
int wlk_vad_stream_run_pcm16(wlk_vad_stream* s, const int16_t* pcm_host, int n_windows, float* probs_host);
/* One call for the chunks of many streams (config 4: 8 sessions with VAC on, one tick): one upload, three launches (stage
 * the streams' [context | chunk] runs, the per-window front end over all windows, the recurrent cell with one workgroup
 * per stream), one download, one synchronise.  A wlk_vad_group holds only scratch: (h, c) and the 64-sample context stay
 * in each wlk_vad_stream, and a stream's probabilities and state have the bits a wlk_vad_stream_run of the same chunk
 * gives, whatever is stacked beside it - so a stream may go through solo and group calls in any order.
 * streams[i] consumes n_windows[i] x 512 samples; pcm_host holds the streams' chunks back to back in that order, all
 * fp32 or all int16 (sample_format); probs_host receives sum(n_windows) probabilities in the same order.
 * Rejected before anything is enqueued, so that every stream keeps its state and context: a NULL pointer, an unknown
 * sample_format, n_streams < 1, a window count < 1, the same stream twice, a stream created from another wlk_vad: WLK_ERR_ARG;
 * n_streams > max_streams, sum(n_windows) > max_windows_total: WLK_ERR_CAPACITY.
 * Calls are synchronous.  A stream is in at most one call at a time, solo or group (the rule of wlk_vad_stream_run); a
 * group serves one call at a time. */
#define WLK_VAD_F32 0
#define WLK_VAD_S16 1
typedef struct wlk_vad_group wlk_vad_group;
int wlk_vad_group_create(wlk_vad* m, int max_streams /* 1..64 */, int max_windows_total /* 1..4096 */, wlk_vad_group** out);
int wlk_vad_group_run(wlk_vad_group* g, wlk_vad_stream* const* streams, const int32_t* n_windows, int n_streams,
                      const void* pcm_host, int sample_format, float* probs_host);
int wlk_vad_group_destroy(wlk_vad_group* g);

/* ---- diagnostics: one kernel on host data (used by the GPU parity tests only) ---------------- */
const char* wlk_diag_last_error(void);
/* environment switches the library caches on first use (WLK_X3_PERSIST, WLK_X3_BM, WLK_X3_COLMAJOR) are read again at
 * their next use: for tests that flip one inside a process */
int wlk_diag_env_refresh(void);
/* c[m,n] = epilogue(a[m,k](row stride lda, a_floats floats in total) . w[n,k]^T + bias); flags:
 * 1 = exact-erf GELU, 2 = add r[m, ldr] after the activation, 4 = scale columns < scale_cols,
 * 8 = ReLU, 16 = Swish.  force_gemv: 0 = shape-based choice among the MFMA kernels, 1 = weight-streaming kernel
 * (m <= 8), 2 = the k-wave MFMA kernel of under-filled grids (four waves split K of one 32x32 tile), 3 = the 64x64
 * kernel, 4 = the one-tile-per-CU k-pipe kernel, 5 = the "kp" family of the stacked Sortformer steps (k-wave tiles below
 * 512 rows, k-pipe tiles from there on: one per-element arithmetic, so a row's result does not depend on m) */
int wlk_diag_linear(const float* a, int64_t lda, int64_t a_floats, const float* w, const float* bias,
                    const float* r, int64_t ldr, int m, int n, int k, int flags, float scale, int scale_cols,
                    int force_gemv, float* c);
/* ---- NLLB-200 / M2M-100 translation network --------------------------------------------
 * The reference loads it through the third-party `nllw` package (whisperlivekit/core.py:320-329 `load_model`,
 * translation.py / core.py:483-493 `OnlineTranslation`), which wraps the `transformers` M2M-100 (or its CTranslate2
 * conversion); neither is in the reference tree, so these entry points replace what that backend executes: the encoder
 * over a source sentence, decoder steps with a KV cache, the tied vocabulary projection.  Layout and arithmetic:
 * csrc/nllb.hip.  Packed tensor names: "shared.emb" [vocab][d], "pos.table" [n_positions][d] (the sinusoidal table of
 * M2M100SinusoidalPositionalEmbedding, row = position id), "enc.<i>." / "dec.<i>." + ln1 / qkv (q | k | v rows) / out /
 * [lnx / xq / xkv (k | v rows) / xout] / ln2 / fc1 / fc2 + ".w" / ".b", "enc.ln", "dec.ln". */
typedef struct wlk_nllb_dims {
    int32_t vocab, d_model, heads, ffn, enc_layers, dec_layers;
    int32_t max_src, max_tgt;      /* longest source sentence / target sequence a session is sized for (<= 512 each) */
    int32_t pad_id;                /* padding_idx: position ids start at pad_id + 1 */
    int32_t n_positions;           /* rows of "pos.table" */
    float embed_scale;             /* sqrt(d_model) when config.scale_embedding, else 1 */
} wlk_nllb_dims;
typedef struct wlk_nllb wlk_nllb;
typedef struct wlk_nllb_session wlk_nllb_session;
int wlk_nllb_arena_floats(const wlk_nllb_dims* dims, uint64_t* n_floats);
int wlk_nllb_tensor_lookup(const wlk_nllb_dims* dims, const char* packed_name, uint64_t* offset_floats, uint64_t* numel);
int wlk_nllb_tensor_name(const wlk_nllb_dims* dims, int index, const char** name);
int wlk_nllb_create(const wlk_nllb_dims* dims, int device, wlk_nllb** out);
int wlk_nllb_upload(wlk_nllb* m, const char* packed_name, const float* host, uint64_t numel);
int wlk_nllb_finalize(wlk_nllb* m);
int wlk_nllb_destroy(wlk_nllb* m);
/* rows = hypotheses decoded side by side against one source sentence (1 = greedy, n = beams); own HIP stream */
int wlk_nllb_session_create(wlk_nllb* m, int rows, wlk_nllb_session** out);
int wlk_nllb_session_destroy(wlk_nllb_session* s);
/* M2M100Encoder.forward over one unpadded sentence (n ids, host int64) + the cross-attention K/V of every decoder layer */
int wlk_nllb_encode(wlk_nllb_session* s, const int64_t* src_ids, int32_t n);
/* M2M100Decoder.forward + lm_head for tokens [n_rows][n_tok] (host int64); first != 0 empties the self-attention cache
 * (the decoder prompt, e.g. [</s>, target language]); afterwards one token per row.  Logits of the last position of
 * every row stay on the device for wlk_nllb_topk / wlk_nllb_export.  Asynchronous on the session stream. */
int wlk_nllb_decode(wlk_nllb_session* s, const int64_t* tokens, int32_t n_rows, int32_t n_tok, int32_t first);
/* One single-token step per row after the prompt, with its read-out: wlk_nllb_decode(tokens, n_tok = 1, first = 0) +
 * wlk_nllb_topk(k) as ONE graph replay (inputs read from / results written to a host-coherent block by the kernels
 * themselves: no copy nodes).  Synchronous. */
int wlk_nllb_step(wlk_nllb_session* s, const int64_t* tokens, int32_t n_rows, int32_t k, float* logprobs, int32_t* ids);
/* beam bookkeeping: row i of the self-attention cache becomes the old row source_rows[i] */
int wlk_nllb_kv_reorder(wlk_nllb_session* s, const int32_t* source_rows, int32_t n_rows);
/* log_softmax(logits) of the latest decode, the k (<= 16) best per row, descending: [rows][k].  k > 8 takes the wide
 * kernel (vocabularies of at most 262144 tokens, else WLK_ERR_ARG; a row with fewer than k finite logits fills up with
 * (-inf, -1)); its ranks 0..7 are bit for bit those of k = 8. */
int wlk_nllb_topk(wlk_nllb_session* s, int32_t k, float* logprobs, int32_t* ids);
/* Beam step without moving the cache: row i continues the hypothesis that row source_rows[i] held after the
 * previous step, is fed tokens[i], and the k (1..16) best continuations of every row come back - the table update, the
 * decoder step (self-attention through the ancestry table) and the top-k as ONE graph replay.  Synchronous.  Needs
 * max_tgt <= 512.  The first such step after wlk_nllb_decode with first = 1 starts from rows that hold their own history;
 * once one has run, wlk_nllb_decode with first = 0, wlk_nllb_step and wlk_nllb_kv_reorder return WLK_ERR_STATE until the
 * next wlk_nllb_decode with first = 1 or wlk_nllb_encode (wlk_nllb_topk and wlk_nllb_export stay valid). */
int wlk_nllb_step_beam(wlk_nllb_session* s, const int64_t* tokens /*[n_rows]*/, const int32_t* source_rows /*[n_rows]*/,
                       int32_t n_rows, int32_t k /*1..16*/, float* logprobs, int32_t* ids);
/* number of ancestry steps the session has run since it was created */
int wlk_nllb_session_beam_stats(wlk_nllb_session* s, uint64_t* ancestry_steps);
/* ---- AlignAtt streaming translation (opt-in): which source position a target token was produced from, read
 * off the decoder's own cross-attention.  A session that never sets heads runs exactly the steps above.
 * layer_head_pairs = n x (decoder layer, head), n in 1..64; n = 0 switches the read-out off.  WLK_ERR_ARG for a layer or
 * head out of range, a duplicate pair or n > 64. */
int wlk_nllb_session_set_align(wlk_nllb_session* s, const int32_t* layer_head_pairs, int32_t n);
/* wlk_nllb_step + the alignment read-out as ONE graph replay (its own recording, keyed like wlk_nllb_step's on k and the
 * source length; lo / hi / limit travel in a host-coherent block, so one recording serves every window).  Every selected
 * head's softmax row over the source (the cross-attention kernel's exp(s - max) / sum) is kept; per row
 *   p[j]       = (sum of the heads' rows, in the order they were set) * (1 / n)
 *   align_pos  = the position of the largest p[j], lo <= j < hi, the lowest j on an exact tie; -1 for an empty window
 *   align_prob = p[align_pos] (0 for an empty window)
 *   tail_mass  = sum of p[j], j >= limit
 * Same state rules as wlk_nllb_step; WLK_ERR_STATE before heads are set or after an ancestry step; WLK_ERR_ARG unless
 * 0 <= lo, hi <= src_len and 0 <= limit <= src_len.  Synchronous. */
int wlk_nllb_step_align(wlk_nllb_session* s, const int64_t* tokens, int32_t n_rows, int32_t k /*1..8*/, int32_t lo, int32_t hi,
                        int32_t limit, float* logprobs, int32_t* ids, int32_t* align_pos /*[rows]*/, float* align_prob /*[rows]*/,
                        float* tail_mass /*[rows]*/);
/* The AlignAtt decoding loop for a 1-row session, after wlk_nllb_encode of [source language, content..., </s>] (S ids):
 * prompt = [</s>, target language, committed target ids...] (n_prompt >= 2, else WLK_ERR_ARG); prompt[:-1] is prefilled
 * (wlk_nllb_decode, first = 1: no alignment rows), prompt[-1] and every later token go through the align step with
 * lo = 1, hi = S - 1, limit = max(n_accessible - threshold, lo).  Each step yields a candidate y (arg-max) and its
 * position a.  Not final: the loop ends WITHOUT emitting y when a < 0 or a >= limit (ATTENTION) or y == eos_id (EOS).
 * Final: only y == eos_id ends it (EOS, not emitted).  Both end after max_new tokens (LENGTH) and when the target context
 * is full (CONTEXT).  out_ids / out_align [max_new]; *n_out tokens were emitted. */
enum { WLK_ALIGN_STOP_ATTENTION = 0, WLK_ALIGN_STOP_EOS = 1, WLK_ALIGN_STOP_LENGTH = 2, WLK_ALIGN_STOP_CONTEXT = 3 };
int wlk_nllb_generate_alignatt(wlk_nllb_session* s, const int64_t* prompt, int32_t n_prompt, int32_t n_accessible,
                               int32_t threshold, int32_t final, int64_t eos_id, int32_t max_new, int64_t* out_ids,
                               int32_t* out_align, int32_t* n_out, int32_t* stop_reason);
/* align steps run and align-step graphs recorded since the session was created */
int wlk_nllb_session_align_stats(wlk_nllb_session* s, uint64_t* align_steps, uint64_t* graph_captures);
/* parity exports: "logits" [rows][vocab] of the latest decode, "enc" [src_len][d_model], "align" [rows][src_len] = p of
 * the latest align step */
int wlk_nllb_export(wlk_nllb_session* s, const char* what, float* host, uint64_t capacity, uint64_t* n_written);
int wlk_nllb_sync(wlk_nllb_session* s);

/* ---- NLLB: up to 8 DIFFERENT sentences per launch chain (csrc/nllb_batch.hip) ---------------------------------------
 * A session above holds ONE sentence (its rows are hypotheses of it).  A batch holds `n_slots` (1..8) slots, each one
 * sentence in flight with its own encoder output, cross K/V, self-attention cache, source length and target length; the
 * stacked work buffers, the row table, the stream and the step graphs belong to the batch.  Greedy decoding of several
 * sentences shares every weight pass: whisperlivekit_amd.nllb.generate_batch.  One caller at a time per batch.  Like
 * sessions, batches are destroyed before their model. */
typedef struct wlk_nllb_batch wlk_nllb_batch;
int wlk_nllb_batch_create(wlk_nllb* m, int n_slots, wlk_nllb_batch** out);
int wlk_nllb_batch_destroy(wlk_nllb_batch* b);
/* Stacked ragged encode of n sentences into the n different slots named: sentence i is src_ids[src_offsets[i] ..
 * src_offsets[i + 1]) (host int64, unpadded, 1..max_src ids each; src_offsets[0] = 0).  One launch chain over all
 * sum(S_i) rows; attention never crosses a sentence.  Each slot's target length returns to 0.  Slots not named keep
 * their state - they may be in the middle of a decode. */
int wlk_nllb_batch_encode(wlk_nllb_batch* b, const int32_t* slots, const int64_t* src_ids, const int32_t* src_offsets, int32_t n);
/* One decoder step over n_rows (slot, token) pairs - at most one row per slot, any subset, any order - as ONE graph
 * replay, with the read-out: row r feeds tokens[r] at its slot's own position against its slot's own caches and source
 * length, and receives the k (<= 8) best log-probabilities / ids, descending: [n_rows][k].  The first step of a slot
 * after its encode feeds the decoder start token at position 0.  Synchronous. */
int wlk_nllb_batch_step(wlk_nllb_batch* b, const int32_t* slots, const int64_t* tokens, int32_t n_rows, int32_t k, float* logprobs,
                        int32_t* ids);
/* the slot's sentence is done: the slot must be encoded again before its next step */
int wlk_nllb_batch_release(wlk_nllb_batch* b, int32_t slot);
/* parity exports of one slot: "enc" [src_len][d_model], "logits" [vocab] of the slot's row in the latest step, "align"
 * [src_len] = the slot's p of the latest align step (WLK_ERR_STATE if the slot was not in it) */
int wlk_nllb_batch_export(wlk_nllb_batch* b, int32_t slot, const char* what, float* host, uint64_t capacity, uint64_t* n_written);
/* diagnostics: the ragged cross-attention kernel alone - queries q_host [n_rows][d_model] (pre-scaled) against decoder
 * layer `layer`'s cross K/V of the encoded slots named, out_host [n_rows][d_model] */
int wlk_nllb_batch_cross_attention(wlk_nllb_batch* b, const int32_t* slots, int32_t n_rows, int32_t layer, const float* q_host,
                                   float* out_host);
int wlk_nllb_batch_sync(wlk_nllb_batch* b);
/* ---- AlignAtt through the stacked batch (opt-in): up to 8 streaming sessions per decoder weight pass.  A batch
 * that never sets heads allocates nothing for this and records and replays exactly the step graphs above.
 * The rules of wlk_nllb_session_set_align: n x (decoder layer, head), n = 0 switches the read-out off; WLK_ERR_ARG for a
 * layer or head out of range, a duplicate pair or n > 64.  Nothing is allocated until the first align step. */
int wlk_nllb_batch_set_align(wlk_nllb_batch* b, const int32_t* layer_head_pairs, int32_t n);
/* The prompts of n freshly encoded slots (target length 0) in ONE pass over all sum(P_i) rows: prompt i is
 * prompt_ids[prompt_offsets[i] .. prompt_offsets[i + 1]) (P_i >= 1; prompt_offsets[0] = 0), token p of it at position p of
 * slots[i].  No logits are formed - the token whose logits matter goes through a step afterwards.  Afterwards the slot's
 * target length is P_i.  WLK_ERR_STATE for a slot that is not encoded or already holds target tokens, WLK_ERR_CAPACITY for
 * P_i > max_tgt - 1, WLK_ERR_ARG for bad ids or a slot named twice; a refused call changes nothing.  Synchronous. */
int wlk_nllb_batch_prefill(wlk_nllb_batch* b, const int32_t* slots, const int64_t* prompt_ids, const int32_t* prompt_offsets,
                           int32_t n);
/* wlk_nllb_batch_step + the alignment read-out of wlk_nllb_step_align per row, as ONE graph replay: row r reads its own
 * source length and its own window lo[r] | hi[r] | limit[r] (host-coherent block), so one recording per row count - kept
 * apart from wlk_nllb_batch_step's, dropped when the head set or k changes - serves every mix of source lengths, windows
 * and slots.  State rules of wlk_nllb_batch_step, plus WLK_ERR_STATE before heads are set or on a slot whose target length
 * is 0, and WLK_ERR_ARG unless 0 <= lo[r], hi[r] <= src_len_r and 0 <= limit[r] <= src_len_r for every row. */
int wlk_nllb_batch_step_align(wlk_nllb_batch* b, const int32_t* slots, const int64_t* tokens, int32_t n_rows, int32_t k /*1..8*/,
                              const int32_t* lo /*[n_rows]*/, const int32_t* hi /*[n_rows]*/, const int32_t* limit /*[n_rows]*/,
                              float* logprobs, int32_t* ids, int32_t* align_pos /*[n_rows]*/, float* align_prob /*[n_rows]*/,
                              float* tail_mass /*[n_rows]*/);
/* align steps run and align-step graphs recorded since the batch was created */
int wlk_nllb_batch_align_stats(wlk_nllb_batch* b, uint64_t* align_steps, uint64_t* graph_captures);
/* Draft verification (opt-in).  For n freshly encoded slots (target length 0): ids_i = ids[offsets[i] .. offsets[i+1])
 * = [decoder start, forced first token, d_0 .. d_{n_d-1}]  (P_i = 2 + n_d >= 2, no eos among them).
 * ONE stacked decoder pass over all sum(P_i) rows (the chain of wlk_nllb_batch_prefill), then per slot:
 *   pick_j  = arg-max over the vocabulary of the logits of row 1 + j, j = 0 .. n_d   (lowest id on an exact tie)
 *   k       = the first j < n_d with pick_j != d_j, n_d if there is none
 *   accepted[i] = k,  next_token[i] = pick_k
 * Afterwards the slot's target length is 2 + k: it continues with wlk_nllb_batch_step(next_token).
 * State / argument rules of wlk_nllb_batch_prefill, plus WLK_ERR_ARG for P_i < 2; a refused call launches nothing and
 * changes nothing.  Synchronous.  A batch that never verifies allocates nothing for this; no graph is recorded. */
int wlk_nllb_batch_verify(wlk_nllb_batch* b, const int32_t* slots, const int64_t* ids, const int32_t* offsets, int32_t n,
                          int32_t* accepted, int64_t* next_token);
/* verify passes run, draft tokens offered and draft tokens accepted since the batch was created */
int wlk_nllb_batch_verify_stats(wlk_nllb_batch* b, uint64_t* passes, uint64_t* draft_tokens, uint64_t* accepted_tokens);

/* ---- word-timestamp alignment ------------------------------------------------------------------
 * Dynamic time warping of a [n_rows tokens, n_cols frames] fp32 cost matrix on `device`: replaces `dtw_cpu`
 * (whisperlivekit/whisper/timing.py:82-105; CUDA counterpart `dtw_cuda` :108-138) under `find_alignment` (:163-243).
 * `trace` receives (n_rows + 1) x (n_cols + 1) step codes, row-major: 0 = diagonal, 1 = up (previous token), 2 = left
 * (previous frame), -1 in row 0 / column 0 - the array dtw_cpu hands to `backtrace` (:58-79).  Same strict comparisons
 * (ties go left) and one fp32 add per cell.  n_rows <= 1024.  Host pointers; synchronous. */
int wlk_dtw(int device, const float* x, int32_t n_rows, int32_t n_cols, int8_t* trace);
/* `log_mel_spectrogram(audio, n_mels, padding)` of a whole recording (whisperlivekit/whisper/audio.py:110-157) as
 * `whisper.transcribe()` computes it once per call (transcribe.py:126: padding = 30 s of zeros): STFT 400 / hop 160 with
 * reflection at both ends of the padded signal, mel filterbank, log10, clamp at (maximum over ALL frames) - 8, (x + 4) / 4.
 * `mel` receives [n_mels][n_frames], n_frames = (n_samples + padding) / 160; mel == NULL only reports n_frames.  Host
 * pointers; the work runs on the session's stream, synchronously.  n_samples + padding must exceed 200. */
int wlk_log_mel(wlk_session* s, const float* pcm, int64_t n_samples, int32_t padding, float* mel, uint64_t capacity_floats,
                int32_t* n_frames);
/* Encode a log-mel SEGMENT instead of the session's audio: `mel` is [n_mels][3000] as `whisper.transcribe()` slices it
 * out of the file's log-mel and hands it to the model / to `find_alignment` (whisperlivekit/whisper/transcribe.py,
 * timing.py:163-171).  Runs encoder + cross-K/V; the session then decodes against it like after wlk_encode.  Host
 * pointer, synchronous upload. */
int wlk_encode_mel(wlk_session* s, const float* mel, int32_t n_frames);
/* The device half of `find_alignment` (whisperlivekit/whisper/timing.py:163-218) on an encoded beam-1 session:
 * `tokens` = [sot sequence (n_sot ids), <|notimestamps|>, text tokens, <|endoftext|>] (n_tokens ids).  One decoder pass
 * over them; token_probs[i] = softmax(logits[n_sot + i, :eot])[text token i]; the alignment heads' cross-attention
 * scores -> softmax over the first num_frames / 2 positions (x qk_scale) -> z-score over the token axis -> median-7
 * along the frames -> head mean -> rows [n_sot, n_tokens - 1) negated = the cost matrix [n_text + 1][num_frames / 2]
 * (copied to `cost` when not NULL) -> dtw: `trace` receives (n_text + 2) x (num_frames / 2 + 1) step codes as wlk_dtw
 * returns them.  Walking the path back and cutting it into words stays on the host (timing.py:216-243).  The session
 * needs a new prefill afterwards (its alignment window holds this call's scores). */
int wlk_find_alignment(wlk_session* s, const int64_t* tokens, int32_t n_tokens, int32_t n_sot, int32_t eot,
                       int32_t num_frames, float qk_scale, float* cost, int8_t* trace, float* token_probs);
/* The alignment-head survey for a checkpoint without a head table (the reference's scripts/determine_alignment_heads.py:
 * 125-160) on an encoded beam-1 session: one teacher-forced decoder pass over `tokens` (n_tokens ids, the caller's
 * [sot sequence, <|notimestamps|>, transcript, <|endoftext|>]), and for EVERY decoder layer, head and token row
 * peak[l][h][p] = max softmax(scores[:num_frames / 2]) = 1 / sum_f exp(s_f - max s) and frame[l][h][p] = the lowest position
 * that attains the maximum (NULL: not wanted); [n_text_layer][n_text_head][n_tokens] each.  The scores are never stored.
 * Does not depend on the model's alignment heads (none set is fine).  WLK_ERR_ARG: NULL argument, beam != 1, n_tokens < 1,
 * num_frames / 2 outside 1 .. n_audio_ctx, a token id out of range; WLK_ERR_CAPACITY: n_tokens > n_text_ctx; WLK_ERR_STATE:
 * not encoded, attached to the batch engine, debug or profiling session - all before anything is launched.  The session
 * needs a new prefill afterwards.  Means and votes over the rows are the host's (whisperlivekit_amd/alignment_heads.py). */
int wlk_head_survey(wlk_session* s, const int64_t* tokens, int32_t n_tokens, int32_t num_frames, float* peak, int32_t* frame);

/* kernel-tuning probe: average microseconds per launch over `reps` back-to-back launches of one linear layer on
 * device-resident pseudo-random operands (same `force_gemv` meaning as wlk_diag_linear) */
int wlk_diag_linear_time(int m, int n, int k, int flags, int force_gemv, int reps, float* us_per_launch);
/* c[m,n] = LayerNorm(a[m,k]; gamma, beta, eps 1e-5) . w[n,k]^T + bias, m <= 8: the fused pre-LN projections
 * of the decode-step (weight-streaming) path.  m > 8 is an error: no MFMA kernel takes the LayerNorm */
int wlk_diag_linear_ln(const float* a, const float* w, const float* bias, const float* gamma, const float* beta,
                       int m, int n, int k, int force_gemv, float* c);
int wlk_diag_layernorm(const float* x, const float* gamma, const float* beta, int rows, int d, float* y);
/* test hook of the engine's stacked prefills (csrc/api.hip: wlk_prefill_group): the prefills of n encoded beam-1 sessions of
 * one model (tokens concatenated, n_tok[i] each) as ONE launch chain; taken[i] = 0 for a session whose prompt does not
 * qualify for the stack (nothing is done for it).  A stacked session ends up exactly as after wlk_decode(first = 1). */
int wlk_diag_prefill_stack(wlk_session** sessions, const int64_t* tokens, const int32_t* n_tok, const int32_t* sot_index, int32_t n,
                           int32_t* taken);
/* prefill chains run by the engine's prefill lane and the sessions stacked in them */
int wlk_engine_prefill_stats(wlk_model* m, uint64_t* batches, uint64_t* sessions);
/* kernel-tuning probe: average microseconds per encoder self-attention launch (pseudo-random qkv) */
int wlk_diag_encoder_attention_time(int t, int d, int n_head, int reps, float* us_per_launch);
/* qkv [t, 3d] with q and k pre-scaled -> softmax(q k^T) v per 64-wide head, out [t, d] */
int wlk_diag_encoder_attention(const float* qkv, int t, int d, int n_head, float* out);
/* Token selection and AlignAtt read-out (csrc/select.hip, csrc/align_body.h) on host data, through ONE chosen route.  The
 * launchers are the ones a decode step uses, unchanged; logits, adjustments and the alignment window are the caller's.
 *   route 0  launch_logsoftmax_topk + launch_alignatt (LDS arg-max where the window fits) [+ launch_token_prob]
 *   route 1  as 0 with the read-out's second stage forced to align_argmax_kernel (no LDS)
 *   route 2  launch_select_fused(early_z = false), the no-speech block riding in its second launch when asked for
 *   route 3  align_zscore_kernel, then launch_select_fused(early_z = true) over those z rows
 *   route 4  launch_logsoftmax_topk + launch_alignatt_rows: row r is a beam-0 session of its own with its own counters
 * Row r of the logits is beam r of the window (n_beam = n_rows).  prefill_rows / n_single / newest_row / content_len are
 * arrays of n_rows entries; routes 0-3 have one set for all rows and return WLK_ERR_ARG when the entries differ.  A route
 * that cannot run the shape (fused form refusing, early form with a no-speech request, counters that leave the ring)
 * returns WLK_ERR_ARG with a message in wlk_diag_last_error(); it never runs another route instead.  ns_token < 0: no
 * no-speech probability (ns_logits / ns_probs may be NULL).  All pointers are host memory; the call is synchronous. */
typedef struct wlk_diag_select_args {
    int32_t route, n_rows, n_vocab, k;
    const float* logits;            /* [n_rows][n_vocab] */
    const int32_t* adj_row;         /* [n_adj] row of the adjustment, < 0 = every row */
    const int32_t* adj_ids;         /* [n_adj] unique per row */
    const float* adj_deltas;        /* [n_adj] added to the logit (-inf suppresses) */
    int32_t n_adj;
    int32_t n_align, ring_rows, T, single_base;
    const float* ring;              /* [n_align][n_rows][ring_rows][T] */
    const int32_t* prefill_rows;    /* [n_rows] window = ring rows [0, prefill_rows) + single_base + [0, n_single) */
    const int32_t* n_single;        /* [n_rows] */
    const int32_t* newest_row;      /* [n_rows] ring row of the newest query row */
    const int32_t* content_len;     /* [n_rows] the arg-max runs over frames [0, content_len) */
    int32_t ns_token;
    const float* ns_logits;         /* [n_rows][n_vocab] */
    float* top_logprobs;            /* out [n_rows][k] */
    int32_t* top_ids;               /* out [n_rows][k] */
    int32_t* frames;                /* out [n_rows] */
    float* attn_last;               /* out [n_rows][T] head mean of the median-filtered z rows */
    float* z;                       /* out [n_rows][n_align][T] */
    float* ns_probs;                /* out [n_rows] */
    float* logits_out;              /* out [n_rows][n_vocab] the logits as the call left them in memory (adjusted) */
} wlk_diag_select_args;
int wlk_diag_select(const wlk_diag_select_args* args);
/* log_softmax + top-k alone on host logits [n_rows][n_vocab] through one chosen form, on a stream of its own; synchronous.
 *   form 0  launch_logsoftmax_topk (k in [1, 8], no adjustments)
 *   form 1  launch_logsoftmax_topk_wide (k in [1, 16], n_vocab <= 262144)
 * A form that refuses the shape returns WLK_ERR_ARG; the other form never runs in its place.  n_rows in [1, 64]. */
int wlk_diag_topk(const float* logits, int32_t n_rows, int32_t n_vocab, int32_t k, int32_t form /*0 existing, 1 wide*/,
                  float* logprobs, int32_t* ids);
/* The NLLB alignment read-out kernel alone (csrc/nllb.hip, through its production launcher) on host data
 * probs [n_align][rows][S]: p_out [rows][S], pos / prob / mass [rows] as wlk_nllb_step_align defines them.  n_align in
 * [1, 64], rows in [1, 8], S in [1, 512], 0 <= lo, hi <= S, 0 <= limit <= S; anything else returns WLK_ERR_ARG before any
 * upload.  Synchronous, on a stream of its own. */
int wlk_diag_nllb_align(const float* probs, int32_t n_align, int32_t rows, int32_t S, int32_t lo, int32_t hi, int32_t limit,
                        float* p_out, int32_t* pos, float* prob, float* mass);
/* The RAGGED read-out of a stacked align step (csrc/nllb_batch.hip, through its production launcher) on host data
 * probs [n_align][rows][stride]: row r has its own length S[r] (1..stride) and window lo[r] | hi[r] | limit[r]; p_out
 * [rows][stride] is written at [r][0 .. S[r]) only, pos / prob / mass [rows].  n_align in [1, 64], rows in [1, 8], stride in
 * [1, 512], 0 <= lo, hi <= S, 0 <= limit <= S per row - anything else is refused (WLK_ERR_ARG) before any upload. */
int wlk_diag_nllb_align_rows(const float* probs, int32_t n_align, int32_t rows, int32_t stride, const int32_t* S,
                             const int32_t* lo, const int32_t* hi, const int32_t* limit, float* p_out, int32_t* pos, float* prob,
                             float* mass);
/* The greedy pick of a draft verification alone (csrc/nllb_batch.hip: nllb_verify_pick_rows_kernel through its production
 * launcher, then the fold of its slice partials) on host logits [n_rows][n_vocab]: picks[r] = the arg-max of row r (lowest id
 * on a tie: rank 0 of wlk_diag_topk, form 0), match[r] = (picks[r] == targets[r]).  n_rows in [1, 128], n_vocab in
 * [1, 2^20]; anything else returns WLK_ERR_ARG before any upload.  Synchronous, on a stream of its own. */
int wlk_diag_nllb_verify_pick(const float* logits, int32_t n_rows, int32_t n_vocab, const int32_t* targets, int32_t* picks,
                              int32_t* match);
/* The decoder's attention stage (csrc/decoder.hip, the merged out projection of csrc/gemm_f32.hip, the prefill flash
 * kernel of csrc/attention.hip) on host data, through ONE chosen route.  The launchers are the ones a decode step uses,
 * unchanged.  Heads are 64 wide and d = 64 n_head.
 *   self-attention over a cache [cache rows][ctx_len][d] (kcache / vcache), queries in qkv [n_rows n_tok][3 d]:
 *     S0  launch_decoder_self_attention(n_rows, n_tok, offsets[0])
 *     S1  launch_decoder_self_attention_rows: row r reads cache row row_cache[r] with offsets[r]; the caches sit
 *         layer_off floats into their allocation (the floats in front of them are NaN)
 *     S2  launch_decoder_self_attention_anc with the table anc [anc_rows >= n_rows][ctx_len] and offsets[0]
 *   cross-attention of q [n_rows][d] over k / v [n_kv][T][d]; on the device they lie as [T + 1][2][2 d] with layer 0 and
 *   row T filled with NaN, so the row stride is not 2 d and a read past the keys poisons the result:
 *     C0  launch_decoder_cross_attention (raw scores to `scores` when it is given)
 *     C1  launch_decoder_cross_attention_split + merge kernel
 *     C2  as C1 with the query projection folded in: x [n_rows][d], wq [d][d], bq or NULL, gamma, beta, scale
 *     C3  split with merge = false, then launch_gemv with the merged operand (GemmArgs::mg_*) as a decode step fills it:
 *         out row 0 = resid + bo + wo . attention
 *     C4  as C1 through a StepRow table: row r takes key / value set row_kv[r] and its own alignment window
 *     C5  launch_prefill_cross_attention with k_splits (1, or 0 = the session default) + launch_ring_softmax
 *   Alignment rows: head_rank [n_head] (rank or -1; NULL = no alignment head) sends head h of query row r to
 *   ring[rank][beam_of_row[r]][ring_row[r]][0..T).  Routes C1 - C4 also return the raw scores [n_rows][n_head][T].
 *   integer and copy operations:
 *     A0  launch_anc_update n_updates times on anc, update u with ctl [u][8] = (src 0..6, fresh) and upd_offsets[u]
 *     G0  launch_kv_gather: vcache[l][b] = kcache[l][row_cache[b]] for positions [0, gather_len), n_layer layers
 *     K0  launch_kv_append(n_rows, n_tok, offsets[0]) of qkv's k | v into kcache / vcache
 *     K1  launch_kv_append_rows with row_cache / offsets [n_rows] / layer_off as in S1
 * kcache, vcache, anc, ring, scores and out are uploaded as the caller filled them and copied back whole: what a route
 * does not address keeps the caller's pattern.  A route that cannot run the shape returns WLK_ERR_ARG with a message in
 * wlk_diag_last_error(), before any launch of the refused kernel; it never runs another route instead.  All pointers are
 * host memory; the call is synchronous. */
enum {
    WLK_DA_S0 = 0, WLK_DA_S1 = 1, WLK_DA_S2 = 2,
    WLK_DA_C0 = 10, WLK_DA_C1 = 11, WLK_DA_C2 = 12, WLK_DA_C3 = 13, WLK_DA_C4 = 14, WLK_DA_C5 = 15,
    WLK_DA_A0 = 20, WLK_DA_G0 = 21, WLK_DA_K0 = 22, WLK_DA_K1 = 23
};
typedef struct wlk_diag_dec_attention_args {
    int32_t route, n_rows, n_tok, d, n_head, ctx_len, T;
    int32_t anc_rows, n_updates, gather_len, n_layer, n_kv, k_splits, n_align, n_beam, ring_rows;
    float scale;                    /* C2 */
    int64_t cache_floats;           /* floats of kcache and of vcache */
    int64_t layer_off;              /* S1, K1 */
    int64_t scores_floats, out_floats;
    const float* qkv;
    float* kcache;                  /* in / out */
    float* vcache;                  /* in / out */
    const int32_t* offsets;         /* [1], or [n_rows] for S1 / K1 */
    const int32_t* row_cache;       /* [n_rows] S1 / K1: cache row of query row r; G0: source rows */
    uint8_t* anc;                   /* in / out [anc_rows][ctx_len] */
    const int32_t* ctl;             /* [n_updates][8] */
    const int32_t* upd_offsets;     /* [n_updates] */
    const float* q;
    const float* k;                 /* [n_kv][T][d] */
    const float* v;
    const int32_t* row_kv;          /* [n_rows] C4 */
    const float* x;
    const float* wq;
    const float* bq;
    const float* gamma;
    const float* beta;
    const float* wo;                /* C3 [d][d] */
    const float* bo;
    const float* resid;             /* C3 [d] */
    const int32_t* head_rank;
    const int32_t* ring_row;        /* [n_rows] */
    const int32_t* beam_of_row;     /* [n_rows] */
    float* ring;                    /* in / out [n_align][n_beam][ring_rows][T] */
    float* scores;                  /* in / out [scores_floats] */
    float* out;                     /* in / out [out_floats] */
} wlk_diag_dec_attention_args;
int wlk_diag_dec_attention(const wlk_diag_dec_attention_args* args);
/* ONE kernel of csrc/sortformer.hip on host data through its production launcher, unchanged (the Sortformer blocks and the
 * NLLB encoder share the attention).  Every buffer lives on the device in exactly the floats the caller passes and the
 * in / out ones (q, k, v, pos, in, in2, out) are copied back whole, so a caller's guard pattern around the addressed part
 * travels both ways.  Weights have the sizes their kind states.
 *   ATTENTION    out[i] = softmax_j(scale ((q_i + u) . k_j + (q_i + v) . pos[pos_row0 - i + j])) V per head; rows of q / k / v /
 *                out are ldq / ldk / ldv / ldo floats apart, head h at columns [h dh, (h + 1) dh).  pos (or NULL) has pos_rows
 *                rows of ldp floats, bias_u / bias_v (or NULL) [n_head][dh].  n_seg > 0: rows [seg_start[s], + seg_T[s]) are
 *                independent sequences and T is at least the longest.  form 0 = launch_sf_attention's own rule, 1 = one wave
 *                per query (no segments), 2 = matrix cores.
 *   CONV0        in [sum len][F] -> out [sum sub(len)][sub(F)][C], w [C][9], b [C]; sub(n) = (n - 1) / 2 + 1
 *   DWCONV2D     in [sum len][F][C] -> out [sum sub(len)][sub(F)][C], w [9][C], b [C]
 *   GLU_DWCONV   in [sum len][2 d] -> out [sum len][d], w [taps][d], b / bn_mean / bn_invstd / bn_w / bn_b [d]
 *   HEAD         in [T][d] -> out [T][n_spk], w = w1t [d][d] (transposed), b [d], w2 [n_spk][d], b2 [n_spk]
 *   ASSEMBLE     out[r] = scale * (context row in[r] | chunk row of in2): session s has len[s] rows of which the last len2[s]
 *                are its chunk rows, taken from in2 [sum len2][d] in session order
 * n_sess sessions (1 .. 8) of len[s] frames / rows lie one after the other; the segment tables are built from the lengths as a
 * stacked step builds them.  What the launcher or a buffer cannot hold returns WLK_ERR_ARG with a message in
 * wlk_diag_last_error() before anything is uploaded or launched.  All pointers are host memory; the call is synchronous. */
enum {
    WLK_SFK_ATTENTION = 0, WLK_SFK_CONV0 = 1, WLK_SFK_DWCONV2D = 2, WLK_SFK_GLU_DWCONV = 3, WLK_SFK_HEAD = 4, WLK_SFK_ASSEMBLE = 5
};
typedef struct wlk_diag_sf_kernel_args {
    int32_t kind;
    int32_t T, n_head, dh, form, pos_row0, pos_rows, n_seg;     /* ATTENTION (T: HEAD too) */
    int32_t seg_start[8], seg_T[8];
    int32_t n_sess, len[8], len2[8];
    int32_t F, C, d, taps, n_spk;
    float scale;                    /* ATTENTION, ASSEMBLE */
    int64_t ldq, ldk, ldv, ldo, ldp;
    int64_t q_floats, k_floats, v_floats, pos_floats, in_floats, in2_floats, out_floats;
    float* q;                       /* in / out */
    float* k;                       /* in / out */
    float* v;                       /* in / out */
    float* pos;                     /* in / out, or NULL */
    const float* bias_u;
    const float* bias_v;
    float* in;                      /* in / out */
    float* in2;                     /* in / out (ASSEMBLE) */
    const float* w;
    const float* b;
    const float* w2;
    const float* b2;
    const float* bn_mean;
    const float* bn_invstd;
    const float* bn_w;
    const float* bn_b;
    float* out;                     /* in / out [out_floats] */
} wlk_diag_sf_kernel_args;
int wlk_diag_sf_kernel(const wlk_diag_sf_kernel_args* args);
/* ONE linear layer C = epilogue(LayerNorm?(A) W^T + bias) on host data through a production launcher, unchanged, with
 * every operand a launch can carry.  route: 0 = launch_linear's own choice, 1 = launch_gemv, 2 / 3 / 4 = launch_gemm
 * with force_kernel (k-wave, 64x64, k-pipe), 5 .. 8 = launch_gemm_kp as wlk_diag_linear encodes them (5 = its own choice,
 * 6 = 16 x 16 k-wave tiles, 7 / 8 = 32 x 32 k-wave tiles with two buffers / one), 500 + 10 tm + tn = launch_gemm_kp with the
 * k-pipe kernel's tile tm x tn: an instantiated tile and a shape the kp family gives to the k-pipe kernel (k % 128 == 0,
 * k >= 256, m >= 512), anything else is refused.
 *   a [a_floats] rows lda apart, w [n][k], bias [n] or NULL, ln_gamma / ln_beta [k] or NULL (fused LayerNorm of the rows),
 *   c [c_floats] rows ldc apart, arriving as the caller filled it.  Residual (flags & 2): r [r_floats] rows ldr apart, or
 *   with r_is_c the output buffer itself (its preloaded values; ldr = ldc).
 *   kv_mode 1: columns [kv_d, 3 kv_d) of row (beam, t) also go to kcache / vcache [beams][kv_ctx][kv_d] at position
 *   kv_pos + t (rows are [beam][kv_ntok]; the GEMV kernels take kv_ntok = 1 only).  kv_mode 2 (route 1 only): row r
 *   appends to cache kv_row_cache[r] of n_caches caches lying cache_stride floats apart in kcache / vcache, at
 *   kv_layer_off + kv_row_offset[r] * kv_d (the StepRow table is built on the device).
 *   batch > 0: z = 0 .. batch - 1 operand sets at a + a_off[z], c + c_off[z], r + r_off[z] (floats).
 * Every buffer lives on the device in exactly the floats the caller passes and is copied back whole - inputs too - so a
 * guard pattern around the addressed part travels both ways.  What a buffer cannot hold, or what a launcher refuses,
 * returns WLK_ERR_ARG with a message in wlk_diag_last_error() and leaves every buffer untouched; no other route runs
 * instead.  All pointers are host memory; the call is synchronous. */
typedef struct wlk_diag_linear_args {
    int32_t route, m, n, k, flags, scale_cols, scale_period, r_is_c;
    int32_t kv_mode, kv_pos, kv_d, kv_ctx, kv_ntok, n_caches, batch;
    int32_t kv_row_cache[8], kv_row_offset[8];
    float scale;
    int64_t lda, ldr, ldc, kv_layer_off, cache_stride;
    int64_t a_floats, w_floats, bias_floats, ln_floats, r_floats, c_floats, cache_floats;
    int64_t a_off[8], c_off[8], r_off[8];
    float* a;                       /* in / out */
    float* w;                       /* in / out */
    float* bias;                    /* in / out, or NULL */
    float* ln_gamma;                /* in / out [ln_floats], or NULL */
    float* ln_beta;                 /* in / out [ln_floats] */
    float* r;                       /* in / out, or NULL */
    float* c;                       /* in / out */
    float* kcache;                  /* in / out [cache_floats] */
    float* vcache;                  /* in / out [cache_floats] */
} wlk_diag_linear_args;
int wlk_diag_linear_ex(const wlk_diag_linear_args* args);
/* Which kernel launch_gemv takes for m rows of an n x k layer (has_ln: fused LayerNorm; kv_mode as above), as text:
 * "gemv1<UB,RPW,ln|plain,full|part>" for the single-row kernel, "gemv<MR,RPW>" for the staged one.  The answer of the
 * function launch_gemv itself switches on; needs no device.  A shape launch_gemv refuses returns WLK_ERR_ARG and the
 * refusal as text. */
int wlk_diag_gemv_variant(int m, int n, int k, int has_ln, int kv_mode, char* out_text, int cap);
/* Which tiled GEMM kernel a launch of m x n x k takes on route `route` of wlk_diag_linear_ex (0, 2 .. 8, 500 + 10 tm + tn;
 * batch operand sets, has_cache: the fused cache append), as text: "gemm<64,64>", "gemm<32,64>", "kwave<gemm>",
 * "kwave16<gemm>" (launch_gemm), "kwave<kp,2>", "kwave<kp,1>", "kwave16<kp>" (launch_gemm_kp's k-wave forms with two buffers
 * / one / 16 x 16 tiles), "kpipe<tm,tn>" (either launcher).  The answer of the function both launchers launch; needs no
 * device.  What a launcher refuses, a launch the GEMV kernels take and a tile route wlk_diag_linear_ex refuses return
 * WLK_ERR_ARG and the refusal as text. */
int wlk_diag_gemm_plan(int m, int n, int k, int route, int batch, int has_cache, char* out_text, int cap);
/* ONE encoder operator on host data through its production launcher, unchanged.  kind:
 *   WLK_ENC_X3_GEMM    launch_gemm_x3: C = epilogue(A W^T + bias), m x n x k.  a = `in` (fp32 rows ld_in apart, packed on the
 *                      device with launch_x3_pack) or `in3` (an X3 row image, rows 3 ld_in apart); w [n][k] (launch_x3_pack_w);
 *                      bias [n] at bias + bias_off, or NULL; flags / scale / scale_cols / scale_period as GemmFlags; residual
 *                      r rows ldr apart, or with r_is_c the result itself.  form 0: fp32 rows ld_out apart in `out`; form 1:
 *                      the fc1 row image in out3 (x3_out, rows 3 ld_out3 apart, vt_col0 >= n); form 2: the attention operand
 *                      image in out3 (columns below vt_col0 as rows 3 ld_out3 apart, the others transposed at vt_off with
 *                      rows 3 vt_ld apart).  batch >= 1 fills a pointer table as the encoder does; 0 uses plain pointers.
 *   WLK_ENC_LN         LayerNorm of m rows of n = d features (gamma = w, beta = bias); form 0: launch_layernorm(_batched),
 *                      fp32 rows ld_out apart; form 1: launch_layernorm_x3(_batched), the X3 row image (rows 3 ld_out3 apart).
 *   WLK_ENC_ATTENTION  encoder self-attention of m = T frames, n = d = 64 n_head; form 0: launch_encoder_attention(_batched)
 *                      on fp32 qkv [T][3 d], out [T][d]; form 1: launch_encoder_attention_x3 on `in` (packed with
 *                      launch_x3_pack_qkv) or on in3 (the operand image form 2 of the GEMM writes), fp32 rows ld_out apart or,
 *                      with x3_out, the X3 row image in out3 (rows 3 ld_out3 apart).
 *   WLK_ENC_PACK       launch_x3_pack of m rows of n columns: in (ld_in) -> out3 (ld_out3).
 * batch > 0: operand set z lies at in + in_off[z] (floats), in3 + in3_off[z], out + out_off[z], out3 + out3_off[z] (16-bit
 * words), r + r_off[z].  X3 images travel as raw 16-bit words; nothing is zeroed for the caller.  Every buffer lives on the
 * device in exactly the elements the caller passes and is copied back whole - inputs too.  What a buffer cannot hold, or
 * what a launcher refuses (by the launcher's own check function, its own text), returns WLK_ERR_ARG with a message in
 * wlk_diag_last_error() before anything is uploaded or launched; no other route runs instead.  All pointers are host memory; the call is synchronous. */
#define WLK_ENC_X3_GEMM 0
#define WLK_ENC_LN 1
#define WLK_ENC_ATTENTION 2
#define WLK_ENC_PACK 3
typedef struct wlk_diag_enc_op_args {
    int32_t kind, form, m, n, k, n_head, flags, scale_cols, scale_period, r_is_c, x3_out, batch, vt_col0;
    float scale;
    int64_t ld_in, ld_out, ld_out3, ldr, vt_off, vt_ld, bias_off;
    int64_t in_floats, in3_elems, w_floats, bias_floats, r_floats, out_floats, out3_elems;
    int64_t in_off[8], in3_off[8], r_off[8], out_off[8], out3_off[8];
    float* in;                      /* in / out, or NULL */
    uint16_t* in3;                  /* in / out, or NULL */
    float* w;                       /* in / out */
    float* bias;                    /* in / out, or NULL */
    float* r;                       /* in / out, or NULL */
    float* out;                     /* in / out, or NULL */
    uint16_t* out3;                 /* in / out, or NULL */
} wlk_diag_enc_op_args;
int wlk_diag_enc_op(const wlk_diag_enc_op_args* args);
/* The device half of find_alignment behind the vocabulary projection (csrc/word_align.hip) on host data, through its
 * production launcher launch_word_align, unchanged: token probabilities softmax(logits[i][:n_cols])[targets[i]] of the
 * n_text = P - n_sot - 2 rows of logits (rows ld apart); w = softmax(qk_scale * ring[a][r][:F]) of the rows r < P of the raw
 * scores ring [n_align][ring_rows][T]; in place its z-score over the P rows; cost [n_text + 1][F] = minus the head mean of
 * the width-7 median of the rows n_sot .. P - 2; trace [(n_text + 2)][F + 1] = dtw's step codes.  last_stage stops the
 * chain after WLK_WA_SOFTMAX, _ZSCORE (w holds z), _COST or _DTW; cost / trace may be NULL for the stages that do not write
 * them.  Every buffer lives on the device in exactly the elements the caller passes and is copied back whole - inputs too.
 * What a buffer cannot hold, or what the launcher's check function refuses (its own text), returns WLK_ERR_ARG with a
 * message in wlk_diag_last_error() before anything is uploaded.  All pointers are host memory; the call is synchronous. */
#define WLK_WA_SOFTMAX 0
#define WLK_WA_ZSCORE 1
#define WLK_WA_COST 2
#define WLK_WA_DTW 3
typedef struct wlk_diag_word_align_args {
    int32_t P, F, T, ring_rows, n_align, n_sot, n_cols, last_stage;
    float qk_scale;
    int64_t ld;
    int64_t ring_floats, logits_floats, targets_n, w_floats, cost_floats, probs_floats, trace_bytes;
    float* ring;                    /* in / out */
    float* logits;                  /* in / out */
    int32_t* targets;               /* in / out [targets_n] */
    float* w;                       /* in / out */
    float* cost;                    /* in / out, or NULL */
    float* probs;                   /* in / out */
    int8_t* trace;                  /* in / out, or NULL */
} wlk_diag_word_align_args;
int wlk_diag_word_align(const wlk_diag_word_align_args* args);
/* The kernel of wlk_head_survey (csrc/head_survey.hip) on host data, through its launcher launch_head_survey, unchanged:
 * q [n_layer][P] rows of ldq floats (the scaled queries, head h in columns 64 h ..), k = Tk rows of ldkv >= n_layer x 2 x 64
 * n_head floats with layer l's keys at column l x 2 x 64 n_head (the session's cross K|V layout); for every (layer, head,
 * row) over the first F <= Tk keys peak = 1 / sum_f exp(s_f - max s) and frame = the lowest arg-max, [n_layer][n_head][P]
 * each (frame may be NULL).  k_splits forces that many key ranges (whole 128-key trips; more than there are trips: clamped);
 * 0 = the launcher's own choice.  The inputs must be finite in the first F key rows.  Buffers, refusals and
 * synchronisation as wlk_diag_word_align. */
typedef struct wlk_diag_head_survey_args {
    int32_t n_layer, n_head, P, F, Tk, k_splits;
    int64_t ldq, ldkv;
    int64_t q_floats, k_floats, peak_floats, frame_n;
    float* q;                       /* in / out */
    float* k;                       /* in / out */
    float* peak;                    /* in / out */
    int32_t* frame;                 /* in / out, or NULL */
} wlk_diag_head_survey_args;
int wlk_diag_head_survey(const wlk_diag_head_survey_args* args);
/* NLLB's ragged decoder cross-attention (csrc/nllb_batch.hip) on host data through launch_nllb_cross_attention_ragged
 * (align = 0) or launch_nllb_cross_attention_ragged_align (align = 1), unchanged: q [n_rows][d], d = 64 n_head; row r
 * attends to the lengths[r] (1 .. 512) key rows of its block kv + kv_at[r], which holds kv_rows[r] >= lengths[r] rows of
 * ldkv floats with k at kv_off and v at kv_off + d; out [n_rows][d].  The align form (n_rows <= 8) also stores the weights
 * of every head h with head_rank[h] >= 0 to align_probs[head_rank[h]][r][0 .. lengths[r]) ([n_rank][8][align_stride]).
 * Buffers, refusals and synchronisation as wlk_diag_word_align. */
typedef struct wlk_diag_nllb_cross_ragged_args {
    int32_t n_rows, d, n_head, align, n_rank, align_stride;
    int64_t kv_off, ldkv;
    int64_t q_floats, kv_floats, out_floats, probs_floats;
    const int32_t* lengths;         /* [n_rows] */
    const int64_t* kv_at;           /* [n_rows] */
    const int32_t* kv_rows;         /* [n_rows] */
    int32_t* head_rank;             /* [n_head], or NULL */
    float* q;                       /* in / out */
    float* kv;                      /* in / out */
    float* out;                     /* in / out */
    float* align_probs;             /* in / out, or NULL */
} wlk_diag_nllb_cross_ragged_args;
int wlk_diag_nllb_cross_ragged(const wlk_diag_nllb_cross_ragged_args* args);
/* The launch geometry launch_gemm_x3 takes for `batch` sessions (0 = plain pointers) of an m x n x k problem on a device of
 * `cus` compute units, as text: "bm=96|64 banded|plain colmajor|rowmajor persist=.. tiles=MxN nslab=.. slots=.. blocks=..
 * walked=.. max_tiles_per_wg=.. skips_between=0|1" - the answer of the function launch_gemm_x3 itself calls (the WLK_X3_*
 * switches included), with the walk of the kernel's workgroups counted on the host; needs no device. */
int wlk_diag_x3_plan(int m, int n, int k, int batch, int cus, char* out_text, int cap);
/* the VALU wave butterflies of csrc/wave_ops.h (DPP / v_permlane{16,32}_swap) against the __shfl_xor loops they replace,
 * on one wave of 64 floats: ten rows of 64 results each (sum, max, 16-lane sum, xor 1 .. 32 exchanges, arg-max index) */
int wlk_diag_wave_ops(const float* in64, float* out640, float* ref640);
/* the X3 path of the encoder's wide projections (csrc/x3.h, gemm_x3.hip: fp32 operands as three bf16 planes, six bf16
 * MFMAs per fp32 product): C = epilogue(A W^T + bias) with both operands packed on the device; its timing probe; and the
 * LayerNorm that writes its result in that format, unpacked again (bit-identical to wlk_diag_layernorm) */
int wlk_diag_linear_x3(const float* a, const float* w, const float* bias, int m, int n, int k, int flags, float scale,
                       int scale_cols, float* c);
int wlk_diag_linear_x3_time(int m, int n, int k, int flags, int reps, float* us_per_launch);
int wlk_diag_layernorm_x3(const float* x, const float* gamma, const float* beta, int rows, int d, float* y);
/* encoder self-attention through the X3 path (csrc/attention_x3.hip; same contract as wlk_diag_encoder_attention) and
 * its timing probe */
int wlk_diag_encoder_attention_x3(const float* qkv, int t, int d, int n_head, float* out);
int wlk_diag_encoder_attention_x3_time(int t, int d, int n_head, int reps, float* us_per_launch);
/* Every 16-byte request that workgroup (head, q_tile) of the X3 attention kernel makes on the operand image of t rows of a
 * d-wide model, computed on the host by the functions the kernel itself calls (no launch, needs no device).  src_off[i]: byte
 * offset from the start of the image; lds_off[i]: the byte of the 3 x 49 152 byte LDS ring it lands at, or -1 for a load into
 * registers.  Order: the Q fragments [thread 0 .. 511][feature step 0 / 1][plane 0 .. 2], then the LDS-DMA requests
 * [ring step 0 .. n_steps + 1][wave 0 .. 7][piece 0 .. 5][lane 0 .. 63] (n_steps = pairs of 32-key tiles; the last two steps
 * re-fetch the last pair).  At most cap entries are written, *n_out is their full count, *image_bytes (may be NULL) the size of
 * the image.  WLK_ERR_ARG for a shape the launcher refuses or a workgroup the grid does not have. */
int wlk_diag_attn_x3_addresses(int t, int d, int n_head, int head, int q_tile, int64_t* src_off, int32_t* lds_off, int64_t cap,
                               int64_t* n_out, int64_t* image_bytes);
/* the production operand route of that attention (qkv projection with the X3 epilogue -> attention) against the diagnostic
 * one (fp32 projection -> x3 pack -> attention) on x [t][d], w [3 d][d], bias [3 d]: the two outputs [t][d] must be equal
 * bit for bit */
int wlk_diag_qkv_x3_attention(const float* x, const float* w, const float* bias, int t, int d, int n_head, float scale,
                              float* out_epilogue, float* out_packed);

#ifdef __cplusplus
}
#endif
#endif /* WLK_HIP_H */
