#!/usr/bin/env python
"""NLLB AlignAtt through the stacked batch: what the alignment read-out costs a stacked step, and what one update
tick of 8 streaming sessions costs stacked against session by session.  NLLB-200-distilled-600M shape, seeded weights with
the cross-attention gain of the alignment fixture (tests/nllb_align_standin.py align_gain_state_dict: positions are not
flat), the 16 heads of decoder layer 6, 24-token sources (GPU only; run with the profiler off).

    python scripts/nllb_alignatt_batch_probe.py > profiles/nllb_alignatt_batch_mi355x.txt

(a) `wlk_nllb_batch_step` against `wlk_nllb_batch_step_align` (k = 1) at 1, 4 and 8 rows, alternating in one process on twin
    batches of one model: both are re-primed (encode, start token), then STEPS stacked steps each are timed with a host clock
    (both calls are synchronous); ROUNDS rounds after a warm-up of both; median (best) microseconds per step.  The twins'
    top-1 ids and log-probabilities are compared bit for bit.
(b) one update tick of 8 sessions, each with its own 24-token source: eight 1-row sessions running
    `nllb.generate_alignatt` (the library loop) one after another - the route before DESIGN 22 - against ONE
    `nllb.generate_alignatt_batch` of the same eight requests; alternating, ROUNDS rounds after a warm-up; for committed
    prefixes of 0, 8 and 24 target ids and for runs of 1 and of 8 emitted tokens (final = True with max_new_tokens = 1 / 8, so
    the run length does not hang on the seeded weights' alignment).  ms per tick, median (best); the two routes' outputs are
    compared.
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SRC_LEN, STEPS, ROUNDS, N_SESSIONS = 24, 32, 9, 8
LANG_SRC, LANG_TGT = 256047, 256057


def main():
    from nllb_align_standin import align_gain_state_dict
    from whisperlivekit_amd import _lib, nllb
    if _lib.device_count() < 1:
        raise SystemExit("nllb_alignatt_batch_probe: no HIP device (there is nothing to measure without one)")
    cfg = nllb.NLLB_200_DISTILLED_600M
    model = nllb.HipNllbModel.from_hf_state_dict(cfg, align_gain_state_dict(cfg, 1), device=0, max_src=64, max_tgt=64)
    rng = np.random.default_rng(3)
    srcs = [np.concatenate([[LANG_SRC], rng.integers(4, 250000, size=SRC_LEN - 2), [2]]).astype(np.int64) for _ in range(N_SESSIONS)]
    heads = nllb.default_alignment_heads(cfg)
    print(f"# NLLB-200-distilled-600M shape, seeded weights (align_gain_state_dict(cfg, 1)), fp32; {N_SESSIONS} sources of {SRC_LEN} "
          f"tokens; {len(heads)} alignment heads (decoder layer {heads[0][0]})")

    # (a) the stacked step alone
    plain, align = model.new_batch(8), model.new_batch(8)
    align.set_alignment_heads(heads)

    def run(batch, aligned, R):
        slots = list(range(R))
        for s in slots:
            batch.release(s)
        batch.encode(slots, srcs[:R])
        batch.step(slots, [2] * R, 1)
        toks, ids, lps = [LANG_TGT] * R, [], []
        batch.sync()
        a = time.perf_counter()
        for _ in range(STEPS):
            if aligned:
                lp, i, _pos, _prob, _mass = batch.step_align(slots, toks, 1, [1] * R, [SRC_LEN - 1] * R, [SRC_LEN - 3] * R)
            else:
                lp, i = batch.step(slots, toks, 1)
            toks = [int(t) if int(t) != cfg.pad_token_id else 1234 for t in i[:, 0]]       # (a padding id cannot be fed)
            ids.append(toks)
            lps.append(lp[:, 0].copy())
        dt = time.perf_counter() - a
        return 1e6 * dt / STEPS, ids, np.asarray(lps, np.float32)

    print("| rows | wlk_nllb_batch_step us/step | wlk_nllb_batch_step_align us/step | difference us | ratio | same top-1 bits |")
    print("|---:|---:|---:|---:|---:|---:|")
    for R in (1, 4, 8):
        for _ in range(2):                                                   # code objects, graph recordings
            run(plain, False, R), run(align, True, R)
        t = {False: [], True: []}
        same = True
        for _ in range(ROUNDS):
            us_p, ids_p, lp_p = run(plain, False, R)
            us_a, ids_a, lp_a = run(align, True, R)
            t[False].append(us_p), t[True].append(us_a)
            same = same and ids_p == ids_a and np.array_equal(lp_p.view(np.uint32), lp_a.view(np.uint32))
        med = {k: statistics.median(v) for k, v in t.items()}
        r = dict(rows=R, step_us_median=round(med[False], 1), step_us_best=round(min(t[False]), 1),
                 step_align_us_median=round(med[True], 1), step_align_us_best=round(min(t[True]), 1),
                 align_minus_step_us=round(med[True] - med[False], 1), align_over_step=round(med[True] / med[False], 4),
                 steps_per_round=STEPS, rounds=ROUNDS, bitwise_equal_topk=bool(same))
        print(json.dumps(dict(stacked_step=r)))
        print(f"| {R} | {r['step_us_median']} ({r['step_us_best']}) | {r['step_align_us_median']} ({r['step_align_us_best']}) | "
              f"{r['align_minus_step_us']} | {r['align_over_step']} | {r['bitwise_equal_topk']} |")
    print(json.dumps(dict(align_graph_captures=align.align_stats()["graph_captures"], plain_align_stats=plain.align_stats())))
    plain.close()
    for s in range(8):
        align.release(s)

    # (b) one update tick of 8 sessions
    sessions = [model.new_session(1) for _ in range(N_SESSIONS)]
    for s in sessions:
        s.set_alignment_heads(heads)
    batch = align
    greedy = [nllb.generate_alignatt(sessions[i], srcs[i], LANG_TGT, n_accessible=SRC_LEN, threshold=0, final=True, max_new_tokens=32)[0]
              for i in range(N_SESSIONS)]
    print(json.dumps(dict(greedy_lengths=[len(g) for g in greedy])))
    rows = []
    for committed in (0, 8, 24):
        for emitted in (1, 8):
            reqs = [(srcs[i], LANG_TGT, greedy[i][:committed], SRC_LEN, 0, True, emitted) for i in range(N_SESSIONS)]

            def by_sessions():
                a = time.perf_counter()
                out = [nllb.generate_alignatt(sessions[i], src, bos, committed=c, n_accessible=n, threshold=thr, final=f, max_new_tokens=m)
                       for i, (src, bos, c, n, thr, f, m) in enumerate(reqs)]
                return 1e3 * (time.perf_counter() - a), out

            def stacked():
                a = time.perf_counter()
                out = nllb.generate_alignatt_batch(batch, reqs)
                return 1e3 * (time.perf_counter() - a), out

            for _ in range(2):
                by_sessions(), stacked()
            t_s, t_b, same = [], [], True
            for _ in range(ROUNDS):
                ms_s, out_s = by_sessions()
                ms_b, out_b = stacked()
                t_s.append(ms_s), t_b.append(ms_b)
                same = same and out_s == out_b
            r = dict(committed=committed, max_new=emitted, emitted=[len(o[0]) for o in out_b],
                     sessions_ms_median=round(statistics.median(t_s), 3), sessions_ms_best=round(min(t_s), 3),
                     stacked_ms_median=round(statistics.median(t_b), 3), stacked_ms_best=round(min(t_b), 3),
                     sessions_over_stacked=round(statistics.median(t_s) / statistics.median(t_b), 3), same_outputs=bool(same))
            rows.append(r)
            print(json.dumps(dict(tick=r)))
    print("| committed ids | emitted per session | 8 sessions one after another, ms per tick | one stacked pass, ms per tick | ratio | same outputs |")
    print("|---:|---:|---:|---:|---:|---:|")
    for r in rows:
        print(f"| {r['committed']} | {r['max_new']} | {r['sessions_ms_median']} ({r['sessions_ms_best']}) | {r['stacked_ms_median']} "
              f"({r['stacked_ms_best']}) | {r['sessions_over_stacked']} | {r['same_outputs']} |")
    print(json.dumps(dict(batch_align_stats=batch.align_stats())))
    for s in sessions:
        s.close()
    batch.close()
    model.close()


if __name__ == "__main__":
    main()
