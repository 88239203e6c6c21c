#!/usr/bin/env python
"""NLLB AlignAtt streaming translation: what the alignment read-out costs per decoder step, and what the policy
saves per sentence, NLLB-200-distilled-600M shape, seeded weights (GPU only).

    python scripts/nllb_alignatt_probe.py > profiles/nllb_alignatt_mi355x.txt

(a) `wlk_nllb_step` against `wlk_nllb_step_align` (k = 1, every head of decoder layer 6), alternating in one process on twin
    sessions of one model: both are re-primed with the same prompt, then STEPS single-token steps each are timed with a host
    clock (both calls are synchronous: they end in a stream synchronise); ROUNDS rounds after a warm-up of both; median
    (best) microseconds per step.  The two sessions' top-1 ids and log-probabilities are compared bit for bit.
(b) a scripted 12-word sentence that arrives word by word (a two-word hypothesis tail for the AlignAtt session), through
    `HipOnlineTranslation` (local agreement of whole re-translations) and `HipAlignAttTranslation`: ms per update
    (`process()` call, encoder pass included) and decoder steps per sentence.  The tokenizer is a stand-in (one id per
    word; no SentencePiece model exists offline) and the weights are seeded, so the TEXT means nothing and neither
    alignment heads nor threshold are validated here; the step counts depend on them.
"""
import json
import os
import statistics
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SRC_LEN, STEPS, ROUNDS, MAX_NEW = 24, 48, 7, 48
SENTENCE = "the quick brown fox jumps over the lazy dog near the river."
LANGS = {"eng_Latn": 256047, "fra_Latn": 256057}
TEXT_IDS = 240000


class WordTokenizer:
    """one id per lower-cased word (a stable hash into the text range): [language code] words </s>"""
    unk_token_id = 3

    def __init__(self):
        self.src_lang = "eng_Latn"

    def __call__(self, text):
        ids = []
        for w in text.lower().split():
            h = 0
            for ch in w:
                h = (h * 131 + ord(ch)) % TEXT_IDS
            ids.append(10 + h)
        return types.SimpleNamespace(input_ids=[LANGS[self.src_lang]] + ids + [2])

    def convert_tokens_to_ids(self, tok):
        return LANGS.get(tok, self.unk_token_id)

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(f"w{int(i)}" for i in ids if int(i) not in (0, 1, 2, 3) and int(i) not in LANGS.values())


class Word:
    def __init__(self, text, start, end):
        self.text, self.start, self.end = text, start, end


class HypothesisTail(Word):
    pass


class Counted:
    def __init__(self, sess):
        self._s, self.steps = sess, 0

    def __getattr__(self, name):
        attr = getattr(self._s, name)
        if name != "step":
            return attr

        def counted(*a, **kw):
            self.steps += 1
            return attr(*a, **kw)
        return counted


def stream(model, T):
    """(b) the 12-word stream under both policies"""
    words = [Word(" " + w, round(0.4 * i, 2), round(0.4 * i + 0.4, 2)) for i, w in enumerate(SENTENCE.split())]
    rows = []
    for policy in ("local_agreement", "alignatt", "local_agreement", "alignatt", "local_agreement", "alignatt"):
        tm = T.HipNllbTranslationModel(model, WordTokenizer(), max_new_tokens=MAX_NEW, policy=policy, threshold=2,
                                       hypothesis_tail=(policy == "alignatt"))
        tr = tm.new_session("eng_Latn", "fra_Latn")
        if policy == "local_agreement":
            tr.session = Counted(tr.session)
        per_update = []
        for i, w in enumerate(words):
            items = [w]
            if policy == "alignatt" and i + 1 < len(words):
                items.append(HypothesisTail(" ".join(x.text.strip() for x in words[i + 1:i + 3]), None, None))
            tr.insert_tokens(items)
            a = time.perf_counter()
            tr.process()
            per_update.append(1e3 * (time.perf_counter() - a))
        steps = tr.session.steps if policy == "local_agreement" else tr.session.align_stats()["align_steps"]
        rows.append(dict(policy=policy, updates=len(per_update), ms_per_update_median=round(statistics.median(per_update), 3),
                         ms_per_update_max=round(max(per_update), 3), ms_per_sentence=round(sum(per_update), 2),
                         decoder_steps_per_sentence=int(steps)))
        print(json.dumps(rows[-1]))
        tr.close()
    print("| policy | updates | ms per update, median (max) | ms per sentence | decoder steps per sentence |")
    print("|---|---:|---:|---:|---:|")
    for r in rows[2:]:                                                      # the first pass of each policy warms up
        print(f"| {r['policy']} | {r['updates']} | {r['ms_per_update_median']} ({r['ms_per_update_max']}) | {r['ms_per_sentence']} | "
              f"{r['decoder_steps_per_sentence']} |")


def main():
    from whisperlivekit_amd import _lib, nllb
    from whisperlivekit_amd import translation as T
    if _lib.device_count() < 1:
        raise SystemExit("nllb_alignatt_probe: no HIP device (there is nothing to measure without one)")
    cfg = nllb.NLLB_200_DISTILLED_600M
    model = nllb.HipNllbModel.from_hf_state_dict(cfg, nllb.synth_state_dict(cfg, 1), device=0, max_src=64, max_tgt=64)
    rng = np.random.default_rng(3)
    src = np.concatenate([[256047], rng.integers(4, 250000, size=SRC_LEN - 2), [2]]).astype(np.int64)
    heads = nllb.default_alignment_heads(cfg)
    print(f"# NLLB-200-distilled-600M shape, seeded weights (synth_state_dict(cfg, 1)), fp32; source {SRC_LEN} tokens; "
          f"{len(heads)} alignment heads (decoder layer {heads[0][0]})")

    # (a) the step alone
    plain, align = model.new_session(1), model.new_session(1)
    align.set_alignment_heads(heads)
    prompt = np.asarray([[2, 256057]], np.int64)

    def run(sess, aligned):
        sess.decode(prompt, first=True)
        tok, ids, lps = 1234, [], []
        sess.sync()
        a = time.perf_counter()
        for _ in range(STEPS):
            if aligned:
                lp, i, _pos, _prob, _mass = sess.step_align([tok], 1, 1, SRC_LEN - 1, SRC_LEN - 3)
            else:
                lp, i = sess.step([tok], 1)
            ids.append(int(i[0, 0]))
            tok = ids[-1] if ids[-1] != cfg.pad_token_id else 1234          # (a padding id cannot be fed)
            lps.append(lp[0, 0])
        dt = time.perf_counter() - a
        return 1e6 * dt / STEPS, ids, np.asarray(lps, np.float32)

    for s in (plain, align):
        s.encode(src)
    for _ in range(2):                                                       # code objects, graph recordings
        run(plain, False), run(align, True)
    t = {False: [], True: []}
    same = True
    for _ in range(ROUNDS):
        us_p, ids_p, lp_p = run(plain, False)
        us_a, ids_a, lp_a = run(align, True)
        t[False].append(us_p), t[True].append(us_a)
        same = same and ids_p == ids_a and np.array_equal(lp_p.view(np.uint32), lp_a.view(np.uint32))
    med = {k: statistics.median(v) for k, v in t.items()}
    r = dict(step_us_median=round(med[False], 1), step_us_best=round(min(t[False]), 1), step_align_us_median=round(med[True], 1),
             step_align_us_best=round(min(t[True]), 1), align_minus_step_us=round(med[True] - med[False], 1),
             align_over_step=round(med[True] / med[False], 4), steps_per_round=STEPS, rounds=ROUNDS, bitwise_equal_topk=bool(same),
             align_graph_captures=align.align_stats()["graph_captures"])
    print(json.dumps(dict(step_alone=r)))
    print("| wlk_nllb_step us/step | wlk_nllb_step_align us/step | difference us | ratio | same top-1 bits |")
    print("|---:|---:|---:|---:|---:|")
    print(f"| {r['step_us_median']} ({r['step_us_best']}) | {r['step_align_us_median']} ({r['step_align_us_best']}) | "
          f"{r['align_minus_step_us']} | {r['align_over_step']} | {r['bitwise_equal_topk']} |")
    plain.close(), align.close()

    stream(model, T)
    model.close()


if __name__ == "__main__":
    main()
