"""What the NLLB device beam steps are tested with, shared by the CPU and the GPU test file:

* :class:`StandinNllbSession` - ``OracleNllbSession`` with the ``step_beam`` / ``beam_stats`` of ``HipNllbSession``:
  ``kv_reorder(sources)`` + a one-token ``decode`` + the top-k of the logits (k up to 16) on the CPU oracle, the library's
  state rule, and a log of every call;
* :func:`emulate_wide_topk` - the selection of ``launch_logsoftmax_topk_wide`` step by step in numpy (ids only);
* :func:`planted_rows` - rows that aim at its tie rules and edge cases;
* the beam cases of both golden files.
"""
import numpy as np
import torch

import helpers as H
from oracle.nllb_oracle import OracleNllbSession

KAT = H.golden_npz("nllb_kat.npz")
WIDE = H.golden_npz("nllb_beam_wide_kat.npz")
OLD_WEIGHTS = dict(seed=0, eos_gain=6.0)                      # scripts/gen_golden_nllb.py
WIDE_WEIGHTS = dict(seed=int(WIDE["weights"][0]), eos_gain=int(WIDE["weights"][1]) / 1000.0)


def _kw(row):
    lang, beams, lp1000, es, feos, max_new = (int(v) for v in row)
    return lang, dict(num_beams=beams, max_new_tokens=max_new, length_penalty=lp1000 / 1000.0,
                      early_stopping={0: False, 1: True, 2: "never"}[es], forced_eos_token_id=None if feos < 0 else feos)


def beam_cases():
    """-> [(id, weights, src, forced language, beam_search keywords, transformers' sequence)]: the nine of nllb_kat.npz and
    every case of nllb_beam_wide_kat.npz"""
    out = []
    for bi, row in enumerate(KAT["beam_cases"]):
        lang, kw = _kw(row)
        out.append((f"kat{bi}_b{kw['num_beams']}", "old", KAT[f"beam_src{bi}"], lang, kw, KAT[f"beam_out{bi}"].tolist()))
    for bi, row in enumerate(WIDE["cases"]):
        lang, kw = _kw(row)
        out.append((f"wide{bi}_b{kw['num_beams']}", "wide", WIDE[f"src{bi}"], lang, kw, WIDE[f"out{bi}"].tolist()))
    return out


class StateError(RuntimeError):
    """the stand-in's WLK_ERR_STATE"""


class StandinNllbSession(OracleNllbSession):
    def __init__(self, oracle, rows=1):
        super().__init__(oracle, rows)
        self.log = []
        self.anc_live = False
        self.ancestry_steps = 0

    def _refuse(self, what):
        if self.anc_live:
            raise StateError(f"{what} after an ancestry step")

    def encode(self, src_ids):
        self.log.append(("encode",))
        self.anc_live = False
        super().encode(src_ids)

    def decode(self, tokens, first):
        if not first:
            self._refuse("decode(first=False)")
        self.log.append(("decode", bool(first)))
        super().decode(tokens, first)
        if first:
            self.anc_live = False

    def step(self, tokens, k=1):
        self._refuse("step")
        self.log.append(("step", k))
        OracleNllbSession.decode(self, torch.as_tensor(np.asarray(tokens), dtype=torch.int64).view(-1, 1), first=False)
        return OracleNllbSession.topk(self, k)

    def kv_reorder(self, source_rows):
        self._refuse("kv_reorder")
        self.log.append(("kv_reorder", [int(v) for v in source_rows]))
        super().kv_reorder(source_rows)

    def logits(self):
        self.log.append(("logits",))
        return super().logits()

    def topk(self, k):
        if not 1 <= k <= 16:
            raise ValueError("k must be 1..16")
        self.log.append(("topk", k))
        return super().topk(k)

    def step_beam(self, tokens, sources, k):
        if self.cache is None:
            raise StateError("step_beam before the decoder prompt")
        if not 1 <= k <= 16:
            raise ValueError("k must be 1..16")
        sources = [int(v) for v in sources]
        if len(sources) != self.rows or any(not 0 <= v < self.rows for v in sources):
            raise ValueError("source row out of range")
        if any(int(t) == self.oracle.cfg.pad_token_id for t in np.asarray(tokens).reshape(-1)):
            raise ValueError("padding inside a sequence is not supported")        # the library's WLK_ERR_ARG
        self.log.append(("step_beam", sources, k))
        OracleNllbSession.kv_reorder(self, sources)
        OracleNllbSession.decode(self, torch.as_tensor(np.asarray(tokens), dtype=torch.int64).view(-1, 1), first=False)
        self.anc_live = True
        self.ancestry_steps += 1
        return OracleNllbSession.topk(self, k)

    def beam_stats(self):
        return {"ancestry_steps": self.ancestry_steps}

    def calls(self, name):
        return [e for e in self.log if e[0] == name]


# ----------------------------------------------------------------------------------------------------------------------
# launch_logsoftmax_topk_wide's selection, step by step (csrc/select.hip)
# ----------------------------------------------------------------------------------------------------------------------
N_SLICES, N_THREADS, KEEP, NONE = 64, 256, 16, 0x7FFFFFFF


def _better(av, ai, bv, bi):
    """(av, ai) comes before (bv, bi): value descending, index ascending"""
    return av > bv or (av == bv and ai < bi)


def _slice_list(x, lo, hi, k):
    """the k best of slice [lo, hi): 256 strided owners with 16 register entries each; every owner holds the best entry it
    has left, a round takes the best of the 256, and only the winner's owner rescans its entries for what comes after"""
    val = np.full((N_THREADS, KEEP), -np.inf, np.float32)
    idx = lo + np.arange(N_THREADS)[:, None] + N_THREADS * np.arange(KEEP)[None, :]
    inside = idx < hi
    val[inside] = x[idx[inside]]

    def best_after(t, wv, wi):
        bv, bi = -np.inf, NONE
        for j in range(KEEP):
            v, i = float(val[t, j]), int(idx[t, j])
            after = v < wv or (v == wv and i > wi)
            if v > -np.inf and after and _better(v, i, bv, bi):
                bv, bi = v, i
        return bv, bi

    # the first scan of every owner, vectorised: best finite entry, ties to the lower index (entries ascend with j)
    first = val.argmax(axis=1)
    mine_v = val[np.arange(N_THREADS), first].astype(np.float64)
    mine_i = np.where(mine_v > -np.inf, idx[np.arange(N_THREADS), first], NONE)
    out = []
    for _ in range(k):
        order = np.lexsort((mine_i, -mine_v))
        t = int(order[0])
        wv, wi = float(mine_v[t]), int(mine_i[t])
        out.append((wv if wi != NONE else -np.inf, wi))
        if wi != NONE:
            mine_v[t], mine_i[t] = best_after(t, wv, wi)
    return out


def emulate_wide_topk(logits, k):
    """-> ids [R, k] (int64, -1 where a row has fewer than k finite entries) as the wide kernel selects them"""
    x_all = np.asarray(logits, np.float32)
    R, V = x_all.shape
    per = -(-V // N_SLICES)
    if per > N_THREADS * KEEP:
        raise ValueError("the wide form takes rows of at most 262144 logits")
    ids = np.full((R, k), -1, np.int64)
    for r in range(R):
        lists = [_slice_list(x_all[r], s * per, min(V, s * per + per), k) for s in range(N_SLICES)]
        head = [0] * N_SLICES
        for rank in range(k):                      # the 64-list merge: lane = slice, a lane offers the head of its list
            bv, bi, bs = -np.inf, NONE, -1
            for s in range(N_SLICES):
                if head[s] < k:
                    v, i = lists[s][head[s]]
                    if i != NONE and (bs < 0 or _better(v, i, bv, bi)):
                        bv, bi, bs = v, i, s
            if bs < 0:
                break
            ids[r, rank] = bi
            head[bs] += 1
    return ids


def planted_rows():
    """-> {name: (logits [R, V] float32, k, number of finite entries per row or None)}"""
    rng = np.random.default_rng(5)
    out = {}
    V = 70000                                      # slices of 1094: up to five entries per owner
    per = -(-V // N_SLICES)
    x = (rng.standard_normal((4, V)) * 3).astype(np.float32)
    lo = 7 * per
    x[0, [lo + 3, lo + 3 + 256, lo + 3 + 512]] = 30.0              # inside one owner's entries
    x[1, [lo + 10, lo + 11, lo + 200]] = 30.0                      # across owners of one slice (two waves)
    x[2, [8 * per - 1, 8 * per, 9 * per - 1, 9 * per]] = 30.0      # across slice boundaries
    x[3, [lo + 3, lo + 3 + 256, lo + 10, lo + 11, 8 * per - 1, 8 * per]] = 30.0
    x[3, [5, V - 1]] = 29.0
    out["ties"] = (x, 16, None)
    x = (rng.standard_normal((1, V)) * 3).astype(np.float32)
    x[0, 3 * per + 40 + 13 * np.arange(16)] = 20.0 + rng.permutation(16).astype(np.float32)
    out["all_in_one_slice"] = (x, 16, None)
    V = 262144                                     # slices of 4096: sixteen entries per owner
    x = (rng.standard_normal((1, V)) * 3).astype(np.float32)
    x[0, 21 * 4096 + 77 + 256 * np.arange(16)] = 20.0 + rng.permutation(16).astype(np.float32)
    out["all_in_one_thread"] = (x, 16, None)
    out["empty_slices_v1000"] = ((rng.standard_normal((2, 1000)) * 3).astype(np.float32), 16, None)
    x = np.full((2, 5000), -np.inf, np.float32)
    x[0, [4999, 17, 2500, 18, 0]] = [1.0, 2.0, 2.0, -3.0, 0.5]
    x[1, [100, 101, 102, 103, 104]] = 0.25
    out["five_finite"] = (x, 16, 5)
    return out
