// Host half of one AlignAtt decode loop: see loop.hip.  DecodeJob (beam 1) is shared by wlk_decode_until_stop() and the
// cross-session batch engine; BeamJob (beams 2-7) serves wlk_decode_beam_until_stop().
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/wlk_hip.h"

namespace wlk {

struct DecodeJob {
    wlk_loop_params P;
    std::vector<int64_t> seq;            // context + prompt + tokens generated so far
    int n_before;                        // length of seq when the loop started
    std::vector<int32_t> suppress_ids, blank_ids;
    std::vector<int32_t> step_tokens, step_frames;   // one entry per decode step that selected a token
    std::vector<float> step_sums;        // running sum of log-probs after each step (BeamSearchDecoder's sum_logprobs)
    int produced = 0;
    bool fresh = true;                   // the next decoder forward is the first of this infer (prefill)
    float sum_logprob = 0.f;
    float no_speech_prob = 0.f;
    int last_attend;
    int stop = WLK_STOP_NONE;

    DecodeJob(const wlk_loop_params& p, const int64_t* tokens, int n_tok, const int32_t* suppress, int n_sup,
              const int32_t* blank, int n_blank);
    bool begin_step();                                   // false: the loop is over (stop is set)
    bool no_speech(float prob);                          // true: the loop stops here
    void adjustments(std::vector<int32_t>& ids, std::vector<float>& deltas) const;   // unique ids, additive deltas
    bool consume(const float* top_lp, const int32_t* top_ids, int frame);            // false: the loop is over
    void fill(wlk_loop_result* r) const;
};

// BeamSearchDecoder.update + the loop's stop rules for one audio and B = 2..7 hypotheses (wlk_decode_beam_until_stop,
// wlk_beam_job_*): the restatement of policy.BeamUpdate.update and policy._decode_loop.  `rows` are the B hypotheses in
// rank order; the stop rules look at row 0 and only decide how many of its new tokens the result keeps (`n_keep`).
struct BeamJob {
    wlk_loop_params P;
    int B;
    std::vector<std::vector<int64_t>> rows;          // context + prompt + generated tokens of every hypothesis
    int n_before;
    std::vector<int32_t> suppress_ids, blank_ids;
    std::vector<float> sums;                         // sum_logprobs of every row
    std::vector<int32_t> src;                        // source row of every row in the last update
    std::vector<std::vector<int64_t>> fin_seqs;      // `finished` of this infer (insertion order) and its scores
    std::vector<float> fin_scores;
    std::vector<int32_t> step_tokens, step_frames;
    std::vector<float> step_sums;
    int produced = 0;
    bool fresh = true;
    bool completed = false;
    float no_speech_prob = 0.f;
    int last_attend;
    int n_keep = 0;                                  // new tokens of row 0 the result hands back
    int stop = WLK_STOP_NONE;

    BeamJob(const wlk_loop_params& p, int beam, const int64_t* tokens, int n_tok, const int32_t* suppress, int n_sup,
            const int32_t* blank, int n_blank);
    bool begin_step();
    bool no_speech(float prob);                      // row 0's probability
    void adjustments(std::vector<int32_t>& ids, std::vector<float>& deltas) const;   // from row 0, for all rows
    // top_lp / top_ids: [B][B + 1]; frames: [B] as read before the reorder.  1: goes on, 0: the loop is over,
    // -1: fewer than B live candidates (cannot happen with B + 1 distinct ids per row)
    int consume(const float* top_lp, const int32_t* top_ids, const int32_t* frames);
    void fill(wlk_loop_result* r) const;
};

// blank list (first step) + suppress list + DRY penalty of `seq` as unique ids with additive deltas
void loop_adjustments(const wlk_loop_params& P, const std::vector<int64_t>& seq, bool fresh,
                      const std::vector<int32_t>& blank_ids, const std::vector<int32_t>& suppress_ids,
                      std::vector<int32_t>& ids, std::vector<float>& deltas);

}  // namespace wlk
