#!/usr/bin/env python
"""Stacked NLLB against the one-sentence path, NLLB-200-distilled-600M shape, seeded weights (GPU only):

    python scripts/nllb_batch_probe.py                  (a) and (b) below, N = 1, 2, 4, 8
    python scripts/nllb_batch_probe.py --profile-pass   one stacked pass of 8 sentences and nothing else, to run under
                                                        `rocprofv3 --kernel-trace --stats -- python ...` (c)

(a) the one-sentence way: N sentences one after another through `nllb.generate` on a 1-row session;
(b) `nllb.generate_batch` through an N-slot `HipNllbBatch`;
both on the same model in the same process, alternating, after a warm-up of every shape; each figure is the median of
REPEATS runs (the best is printed beside it).  Tokens per second are summed over the sentences; a pass includes its
encoder work.  Sources are of mixed length, `max_new_tokens` = 48, and the ids of (a) and (b) are compared.
(c) the ragged cross-attention kernel's share of the kernel time of a stacked pass comes from the profiler's table
(scripts/export_profile.py over the rocprofv3 result).
"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SRC_LENS = [24, 6, 40, 11, 58, 17, 9, 31]
MAX_NEW = 48
REPEATS = 5


class Counted:
    """The batch with its steps counted and timed (host clock around a call that ends in a stream synchronise)."""
    def __init__(self, batch):
        self.b, self.model, self.n_slots = batch, batch.model, batch.n_slots
        self.steps = self.rows = 0
        self.step_s = 0.0

    def encode(self, slots, sources):
        self.b.encode(slots, sources)

    def step(self, slots, tokens, k=1):
        a = time.perf_counter()
        out = self.b.step(slots, tokens, k)
        self.step_s += time.perf_counter() - a
        self.steps += 1
        self.rows += len(slots)
        return out

    def release(self, slot):
        self.b.release(slot)


def main():
    from whisperlivekit_amd import _lib, nllb
    if _lib.device_count() < 1:
        raise SystemExit("nllb_batch_probe: no HIP device (there is nothing to measure without one)")
    cfg = nllb.NLLB_200_DISTILLED_600M
    model = nllb.HipNllbModel.from_hf_state_dict(cfg, nllb.synth_state_dict(cfg, 1), device=0, max_src=64, max_tgt=64)
    rng = np.random.default_rng(3)
    sources = [np.concatenate([[256047], rng.integers(4, 250000, size=n - 2), [2]]).astype(np.int64) for n in SRC_LENS]
    langs = [256057 + i for i in range(len(sources))]
    sess = model.new_session(1)
    if "--profile-pass" in sys.argv:
        batch = model.new_batch(8)
        nllb.generate_batch(batch, sources, langs, max_new_tokens=4)              # code objects, graph recording
        out = nllb.generate_batch(batch, sources, langs, max_new_tokens=MAX_NEW)
        print(json.dumps(dict(profile_pass=True, sentences=len(out), new_tokens=sum(len(o) - 1 for o in out))))
        batch.close(); sess.close(); model.close()
        return
    print(f"# NLLB-200-distilled-600M shape, seeded weights (synth_state_dict(cfg, 1)), fp32; source lengths {SRC_LENS}, "
          f"max_new_tokens {MAX_NEW}; median (best) of {REPEATS} runs, (a) and (b) alternating in one process")
    rows = []
    for n in (1, 2, 4, 8):
        src, lang = sources[:n], langs[:n]
        batch = model.new_batch(n)
        for s, l in zip(src, lang):                                               # warm-up of every shape of both ways
            nllb.generate(sess, s, l, max_new_tokens=4)
        nllb.generate_batch(batch, src, lang, max_new_tokens=4)
        seq_s, stk_s, step_ms = [], [], []
        for _ in range(REPEATS):
            a = time.perf_counter()
            want = [nllb.generate(sess, s, l, max_new_tokens=MAX_NEW) for s, l in zip(src, lang)]
            seq_s.append(time.perf_counter() - a)
            cb = Counted(batch)
            a = time.perf_counter()
            got = nllb.generate_batch(cb, src, lang, max_new_tokens=MAX_NEW)
            stk_s.append(time.perf_counter() - a)
            step_ms.append(1e3 * cb.step_s / cb.steps)
        new_tokens = sum(len(o) - 1 for o in want)
        same = sum(1 for g, w in zip(got, want) if g == w)
        r = dict(n=n, new_tokens=new_tokens, identical_sentences=f"{same}/{n}",
                 sequential_tok_s=round(new_tokens / statistics.median(seq_s), 1), sequential_best_tok_s=round(new_tokens / min(seq_s), 1),
                 sequential_ms_per_token=round(1e3 * statistics.median(seq_s) / new_tokens, 3),
                 stacked_tok_s=round(new_tokens / statistics.median(stk_s), 1), stacked_best_tok_s=round(new_tokens / min(stk_s), 1),
                 stacked_ms_per_step=round(statistics.median(step_ms), 3), stacked_steps=cb.steps, stacked_rows=cb.rows,
                 speedup=round(statistics.median(seq_s) / statistics.median(stk_s), 2))
        rows.append(r)
        print(json.dumps(r))
        batch.close()
    print("| N | (a) sequential tok/s | (a) ms/token | (b) stacked tok/s | (b) ms/stacked step | (b)/(a) | same ids |")
    print("|---:|---:|---:|---:|---:|---:|---:|")
    for r in rows:
        print(f"| {r['n']} | {r['sequential_tok_s']} ({r['sequential_best_tok_s']}) | {r['sequential_ms_per_token']} | "
              f"{r['stacked_tok_s']} ({r['stacked_best_tok_s']}) | {r['stacked_ms_per_step']} | {r['speedup']} | {r['identical_sentences']} |")
    sess.close(); model.close()


if __name__ == "__main__":
    main()
