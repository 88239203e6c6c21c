#!/usr/bin/env python
"""Known answers for NLLB draft verification (wlk_nllb_batch_verify) from the repository's own CPU
oracle (oracle/nllb_oracle.py) run in float64: the micro configuration with the weights of tests/golden/nllb_batch_kat.npz,
and per truth the source, the language id, the limit, the greedy ids of `nllb.generate` and - per generated token - the gap
between the best and the second-best logit.

The condition on every truth: minimum gap >= 2e-3, twice tests/test_nllb.py's LOGIT_ATOL, so that no kernel within
tolerance can flip a pick and no test has to allow for ties.  A candidate that misses the gap is REPLACED here (the scan
goes on to the next source); nothing is skipped when the tests run.  What the tests need is asserted before anything is
written: >= 2 truths of >= 12 tokens that end by </s>, >= 3 that stop at their limit, one of those with >= 70 tokens (the
accept kernel's second ballot round), and one truth of about 12 tokens at the 600M shape (weights seed 1, the source seed
found by scanning) whose gap is >= 1e-2, twice the 5e-3 test_hip_600m_shape_matches_the_oracle allows.

Writes tests/golden/nllb_draft_kat.npz.   --skip-600m keeps the 600M entries of the existing file (the scan needs ~6 GB).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BATCH_CASES = (1, 2, 3, 4, 5, 6, 8, 10, 11)      # nllb_batch_kat.npz's cases 0 and 7 keep gaps of 5.6e-4 and 1.0e-4 only
N_EOS, LONG_LIMIT, BIG_LIMIT = 3, 76, 12


def main():
    import torch

    import nllb_draft_cases as DC
    from whisperlivekit_amd import nllb

    torch.set_num_threads(8)
    cfg = DC.CFG
    kat = np.load(os.path.join(ROOT, "tests", "golden", "nllb_batch_kat.npz"))
    seed, eos_gain = int(kat["seed"]), float(kat["eos_gain"])
    o64 = DC.float64_oracle(cfg, nllb.synth_state_dict(cfg, seed, eos_gain))
    truths = []                                   # (src, lang, max_new, ids, gaps)

    def consider(src, lang, max_new, why):
        ids, gaps = DC.greedy_with_gaps(o64, src, lang, max_new)
        ok = float(gaps.min()) >= DC.GAP_MIN
        print(f"{why}: {len(src)} source ids, language {lang}, limit {max_new}: {len(ids)} ids, ends {ids[-1]}, "
              f"min gap {gaps.min():.3g} -> {'gap ok' if ok else 'gap too small: replaced'}")
        return (np.asarray(src, np.int64), lang, max_new, ids, gaps) if ok else None

    for i in BATCH_CASES:
        _n, lang, max_new = (int(v) for v in kat["cases"][i])
        t = consider(kat[f"src{i}"], lang, max_new, f"nllb_batch_kat case {i}")
        assert t is not None and t[3] == kat[f"gen{i}"].tolist(), f"case {i} of nllb_batch_kat.npz no longer qualifies"
        truths.append(t)
    rng = np.random.default_rng(31)

    def random_source(lo, hi):
        src = rng.integers(4, 1900, size=int(rng.integers(lo, hi))).astype(np.int64)
        src[-1] = cfg.eos_token_id
        return src

    found = 0
    for _ in range(200):                          # truths that end by </s> after >= 12 tokens
        t = consider(random_source(6, 40), 1990 + int(rng.integers(0, 10)), 40, "eos scan")
        if t is not None and t[3][-1] == cfg.eos_token_id and 12 <= len(t[3]) < 41:
            truths.append(t)
            found += 1
            if found == N_EOS:
                break
    assert found == N_EOS, "the scan found too few </s>-terminated truths"
    for _ in range(200):                          # one truth of >= 70 tokens that stops at its limit
        t = consider(random_source(10, 60), 1990 + int(rng.integers(0, 10)), LONG_LIMIT, "long scan")
        if t is not None and len(t[3]) == 1 + LONG_LIMIT and t[3][-1] != cfg.eos_token_id:
            truths.append(t)
            break
    else:
        raise AssertionError("the scan found no long truth")

    eos_ended = [t for t in truths if t[3][-1] == cfg.eos_token_id and len(t[3]) < 1 + t[2] and len(t[3]) >= 12]
    at_limit = [t for t in truths if len(t[3]) == 1 + t[2] and t[3][-1] != cfg.eos_token_id]
    assert len(eos_ended) >= 2 and len(at_limit) >= 3 and any(len(t[3]) >= 70 for t in at_limit)
    assert all(len(t[3]) <= DC.MAX_TGT - 1 for t in truths)

    out = {"seed": np.int64(seed), "eos_gain": np.float64(eos_gain), "gap_min": np.float64(DC.GAP_MIN),
           "cases": np.asarray([(t[1], t[2]) for t in truths], np.int64)}
    for i, (src, _lang, _mn, ids, gaps) in enumerate(truths):
        out[f"src{i}"], out[f"gen{i}"], out[f"gap{i}"] = src, np.asarray(ids, np.int64), gaps

    path = os.path.join(ROOT, "tests", "golden", "nllb_draft_kat.npz")
    if "--skip-600m" in sys.argv:
        old = np.load(path)
        for k in old.files:
            if k.startswith("big_"):
                out[k] = old[k]
    else:
        del o64
        big_seed = 1
        big = DC.float64_oracle(DC.BIG_CFG, nllb.synth_state_dict(DC.BIG_CFG, big_seed))
        for src_seed in range(3, 40):
            r = np.random.default_rng(src_seed)
            src = np.concatenate([[256047], r.integers(4, 250000, size=21), [2]]).astype(np.int64)     # language tag, text, </s>
            ids, gaps = DC.greedy_with_gaps(big, src, 256057, BIG_LIMIT)
            print(f"600M shape, source seed {src_seed}: {len(ids)} ids, ends {ids[-1]}, min gap {gaps.min():.3g}")
            if float(gaps.min()) >= DC.BIG_GAP_MIN and len(ids) >= 11:
                out.update(big_seed=np.int64(big_seed), big_src_seed=np.int64(src_seed), big_src=src, big_lang=np.int64(256057),
                           big_max_new=np.int64(BIG_LIMIT), big_gen=np.asarray(ids, np.int64), big_gap=gaps,
                           big_gap_min=np.float64(DC.BIG_GAP_MIN))
                break
        else:
            raise AssertionError("no source seed gave a 600M-shape truth with the required gap")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size < 1024 * 1024, "the fixture must stay under the size limit for committed files"


if __name__ == "__main__":
    main()
