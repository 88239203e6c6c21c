#!/usr/bin/env python
"""NLLB draft verification against draft off, NLLB-200-distilled-600M shape, seeded weights (GPU only):

    python scripts/nllb_draft_probe.py                  the table below
    python scripts/nllb_draft_probe.py --profile-pass   PAIRS updates of ONE caller at 90 % accepted and nothing else, to
                                                        run under `rocprofv3 --kernel-trace --stats -- python ...`
    python scripts/nllb_draft_probe.py --split RESULTS.db
                                                        the kernel time of such a run split into the stacked decoder chain,
                                                        the final LayerNorm, the vocabulary projection, the pick, the accept
                                                        and the steps behind the verify

An update = one `translate_many` request through the model's `NllbStacker`: encode of a 24-token source, then the
30-id hypothesis (max_new_tokens = 29).  Draft off (the yardstick: what the stacker did before drafts) steps every token;
draft on hands the previous hypothesis with a wrong token planted where the accepted share ends (0 / 50 / 90 / 100 % of the
26 draft tokens the limits leave).  1, 4 and 8 callers on as many threads, released together; the time of an update is the
host clock around the caller's `translate_many`, which ends in a stream synchronise.  Alternating pairs (off, on) in one
process after a warm-up of both arms; medians of PAIRS pairs.  The ids of both arms are compared in every pair.
"""
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SRC_LEN, MAX_NEW, PAIRS = 24, 29, 7
SHARES = (0.0, 0.5, 0.9, 1.0)


class Tokenizer:
    """The stacker is driven with ids; the model object only needs a tokenizer to exist."""
    src_lang = "eng_Latn"
    unk_token_id = 3

    def convert_tokens_to_ids(self, tok):
        return 256057


def one_round(stacker, requests):
    """every request on its own thread, released together -> (ids per caller, seconds per caller)"""
    n = len(requests)
    out, secs, errors = [None] * n, [0.0] * n, []
    gate = threading.Barrier(n)

    def work(i):
        try:
            gate.wait()
            a = time.perf_counter()
            out[i] = stacker.translate_many([requests[i]])[0]
            secs[i] = time.perf_counter() - a
        except BaseException as e:       # noqa: BLE001 - reported below
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(n)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    if errors:
        raise errors[0]
    return out, secs


def split(db):
    """A verify pass in the trace: nllb_embed_rows_step_kernel .. the decoder layers .. then per read-out chunk layernorm_kernel,
    the projection's launches and nllb_verify_pick_rows_kernel .. and nllb_verify_accept_kernel at its end."""
    import sqlite3
    c = sqlite3.connect(db)
    rows = c.execute("select name, start, end from kernels order by start").fetchall()
    names = [r[0] for r in rows]
    dur = [(r[2] - r[1]) / 1e3 for r in rows]                           # us
    part = dict(chain=0.0, final_ln=0.0, projection=0.0, pick=0.0, accept=0.0)
    launches = dict(part)
    seen = set()
    accepts = [i for i, n in enumerate(names) if "nllb_verify_accept_kernel" in n]
    prev = -1
    for a in accepts:
        picks = [i for i in range(prev + 1, a) if "nllb_verify_pick_rows_kernel" in names[i]]
        start = max(i for i in range(picks[0]) if "nllb_embed_rows_step_kernel" in names[i])
        kind = {i: "chain" for i in range(start, a)}
        for p in picks:
            ln = max(i for i in range(start, p) if "layernorm_kernel" in names[i])
            kind[p], kind[ln] = "pick", "final_ln"
            for i in range(ln + 1, p):
                kind[i] = "projection"
        kind[a] = "accept"
        for i, k in kind.items():
            part[k] += dur[i]
            launches[k] += 1
            seen.add(i)
        prev = a
    rest = sum(d for i, d in enumerate(dur) if i not in seen)
    n = max(1, len(accepts))
    print(f"# {len(accepts)} verify passes in the trace; kernel time per pass in us (launches per pass)")
    for key, label in (("chain", "stacked decoder chain (embed .. last fc2)"), ("final_ln", "final LayerNorm"),
                       ("projection", "vocabulary projection"), ("pick", "nllb_verify_pick_rows_kernel"),
                       ("accept", "nllb_verify_accept_kernel")):
        print(f"{label:<48} {part[key] / n:9.1f}   ({launches[key] / n:.0f})")
    print(f"{'sum of a verify pass':<48} {sum(part.values()) / n:9.1f}")
    print(f"{'everything else in the trace (encodes, steps), total':<48} {rest:9.1f}")
    proj = sorted({names[i] for a in accepts for i in range(a) if i in seen} & {n for n in names if "gemm" in n.lower()})
    print("# GEMM kernels inside the verify passes:", ", ".join(x[:70] for x in proj[:6]))


def main():
    if "--split" in sys.argv:
        return split(sys.argv[sys.argv.index("--split") + 1])
    from whisperlivekit_amd import _lib, nllb
    from whisperlivekit_amd import translation as T
    if _lib.device_count() < 1:
        raise SystemExit("nllb_draft_probe: no HIP device (there is nothing to measure without one)")
    cfg = nllb.NLLB_200_DISTILLED_600M
    model = nllb.HipNllbModel.from_hf_state_dict(cfg, nllb.synth_state_dict(cfg, 1), device=0, max_src=64, max_tgt=64)
    rng = np.random.default_rng(3)
    sources = [np.concatenate([[256047], rng.integers(4, 250000, size=SRC_LEN - 2), [2]]).astype(np.int64) for _ in range(8)]
    lang = 256057
    tm = T.HipNllbTranslationModel(model, Tokenizer(), max_new_tokens=MAX_NEW, stack=8, draft=True)
    stacker = tm.stacker
    truth = stacker.translate_many([(s, lang, MAX_NEW) for s in sources])
    n_d = len(nllb.clamp_draft(truth[0], MAX_NEW, 64, cfg.eos_token_id))

    def draft(i, share):
        d = list(truth[i])
        n_i = len(nllb.clamp_draft(truth[i], MAX_NEW, 64, cfg.eos_token_id))
        k = int(round(share * n_i))
        if k < n_i:
            d[2 + k] = 1234 if d[2 + k] != 1234 else 1235
        return d

    if "--profile-pass" in sys.argv:
        stacker.translate_many([(sources[0], lang, MAX_NEW, draft(0, 0.9))])          # code objects, buffers, graphs
        for _ in range(PAIRS):
            assert stacker.translate_many([(sources[0], lang, MAX_NEW, draft(0, 0.9))])[0] == truth[0]
        print(json.dumps(dict(profile_pass=True, updates=PAIRS, hypothesis_ids=len(truth[0]), draft_tokens=n_d,
                              stats=tm.batch.verify_stats())))
        tm.close(); model.close()
        return
    print(f"# NLLB-200-distilled-600M shape, seeded weights (synth_state_dict(cfg, 1)), fp32; source {SRC_LEN} ids, hypothesis "
          f"{[len(t) for t in truth]} ids, {n_d} draft tokens; stack=8; alternating pairs ({PAIRS}) after a warm-up of both arms, medians")
    print("callers accepted  off_ms_update  on_ms_update  on/off  off_ms_round  on_ms_round  same_ids")
    rows = []
    for n in (1, 4, 8):
        for share in SHARES:
            off_req = [(sources[i], lang, MAX_NEW) for i in range(n)]
            on_req = [(sources[i], lang, MAX_NEW, draft(i, share)) for i in range(n)]
            one_round(stacker, off_req); one_round(stacker, on_req)                    # warm-up of both arms at this shape
            off_u, on_u, off_r, on_r, same = [], [], [], [], True
            for _ in range(PAIRS):
                a = time.perf_counter()
                want, s_off = one_round(stacker, off_req)
                off_r.append(time.perf_counter() - a)
                a = time.perf_counter()
                got, s_on = one_round(stacker, on_req)
                on_r.append(time.perf_counter() - a)
                off_u.append(statistics.mean(s_off)); on_u.append(statistics.mean(s_on))
                same = same and got == want == truth[:n]
            r = dict(callers=n, accepted=share, off_ms_update=1e3 * statistics.median(off_u), on_ms_update=1e3 * statistics.median(on_u),
                     off_ms_round=1e3 * statistics.median(off_r), on_ms_round=1e3 * statistics.median(on_r), same_ids=same)
            rows.append(r)
            print(f"{n:7d} {100 * share:7.0f}%  {r['off_ms_update']:13.2f} {r['on_ms_update']:13.2f} "
                  f"{r['on_ms_update'] / r['off_ms_update']:7.3f} {r['off_ms_round']:13.2f} {r['on_ms_round']:11.2f}  {same}", flush=True)
    print("# verify stats of the whole run:", json.dumps(tm.batch.verify_stats()))
    tm.close(); model.close()


if __name__ == "__main__":
    main()
