"""Shared by tests/test_gpu_draft_verify.py and tests/test_draft_verify_cpu.py (TEST infrastructure only), modelled on
tests/window_burst_cases.py: the greedy windows whose drafts the verify tests build, the drafts themselves, and an
oracle-backed stand-in for ``HipWindowGroup.verify``.

The model is tiny.en: the stacked decoder pass needs n_text_state >= 256 (every GEMM on the k-wave kernel), so micro.en is
the model the pass REFUSES.  The windows are chosen so that the CPU oracle separates the best allowed token from the
runner-up by >= 1e-3 in log-probability at every step (test_draft_verify_cpu.py asserts it for exactly these seeds), so the
GPU comparisons of token ids need no tie escape."""
import numpy as np

import window_burst_cases as WB
import window_group_cases as WG
from whisperlivekit_amd import _lib, transcribe as TR

MODEL, SEED, MARGIN = "tiny.en", 3, WG.MARGIN
REFUSED_MODEL = "micro.en"

# As window_burst_cases.WINDOWS.  P0 = the initial tokens: 1 (<|startoftranscript|> alone: timestamps on, no prompt), 2 (without
# timestamps), 1 + prompt + 1 with a prompt in front (sot_index = prompt + 1: the no-speech row is not row 0)
WINDOWS = [
    dict(seconds=7.0, seed=5, prompt=0, sample_len=66),                    # P0 = 1: up to 65 rows and beyond
    dict(seconds=4.0, seed=9, prompt=0, sample_len=24, without_timestamps=True),
    dict(seconds=8.5, seed=15, prompt=5, sample_len=60),                   # P0 = 7, sot_index = 6
    dict(seconds=6.0, seed=30, prompt=10, sample_len=12, stamps_and_eot=True),     # [timestamp, <|endoftext|>]: see make_win
    dict(seconds=6.5, seed=13, prompt=0, sample_len=30),
]
TS_WINDOWS = [0, 2, 4]                    # timestamps on, <|endoftext|> suppressed: between them every ts_mode transition
EOT_WINDOW, PROMPT_WINDOW = 3, 2
ALLOWANCE = 5e-4                          # stacked route against solo route, per log-probability (contract 3)


def make_win(index, model, session):
    """window_burst_cases.Win of WINDOWS[index].  stamps_and_eot: under these random weights no window picks <|endoftext|> by
    itself, so this one's suppress list is every token below the timestamps but <|endoftext|> - it opens with a timestamp,
    after which the rules leave <|endoftext|> alone."""
    w = WB.Win(index, WINDOWS[index], model, session)
    if w.spec.get("stamps_and_eot"):
        w.dec.suppressed = [t for t in range(w.dec.tok.timestamp_begin) if t != w.dec.tok.eot]
    return w


def wrong(token):
    """a text token that is not ``token``"""
    return 400 if int(token) != 400 else 401


def sampled(truth_picks, eot):
    """the tokens of a stepwise decode in front of its <|endoftext|>: what a draft may hold"""
    out = []
    for t, _lp in truth_picks:
        if t == eot:
            break
        out.append(int(t))
    return out


def spoiled(tokens, at):
    """``tokens`` with a wrong token at index ``at``"""
    out = [int(t) for t in tokens]
    out[at] = wrong(out[at])
    return out


def expected(truth_picks, draft, eot):
    """what verifying ``draft`` must give when the stepwise decode picked ``truth_picks``: (k, next token) - the common
    prefix and the truth's token there - through the one host statement of the acceptance"""
    k = 0
    while k < len(draft) and k < len(truth_picks) and int(draft[k]) == truth_picks[k][0] and truth_picks[k][0] != eot:
        k += 1
    picks = list(truth_picks[:k + 1]) + [(-1, 0.0)] * (len(draft) - k)       # positions behind k do not matter
    got = TR._accept_draft(picks, draft, eot)
    assert got[0] == k and got[1] == truth_picks[k][0]
    return got


class OracleVerifyGroup(WB.OracleBurstGroup):
    """OracleBurstGroup with ``verify`` / ``verify_fits``: the library's host checks first (a refused call touches nobody),
    then every window is decoded token by token with the oracle, the acceptance is ``transcribe._accept_draft``, and the
    session is left as its own prefill of initial + draft[:k] leaves it.  ``verifies``: per call that got through, the
    (initial tokens, draft tokens, accepted) of its windows."""

    def __init__(self, rows=8, break_at=None, low=9, high=256):
        super().__init__(rows, break_at)
        self.low, self.high = low, high
        self.verifies = []

    def verify_fits(self, n_initial, n_draft):
        return n_initial >= 1 and n_draft >= 1 and self.low <= n_initial + n_draft <= self.high

    def verify(self, windows, want_picks=False):
        def refuse(code, what):
            err = _lib.WlkError(f"wlk_hip error {code}: {what}")
            err.code = code
            raise err
        sessions = [w[0] for w in windows]
        if not 1 <= len(windows) <= self.rows or len(set(map(id, sessions))) != len(sessions):
            refuse(-1, "bad rows")
        for s, initial, draft, _sot, state, _ns in windows:
            if not OracleVerifyGroup.verify_fits(self, len(initial), len(draft)) or state["eot"] in draft:
                refuse(-1, "bad draft")
            if len(initial) + len(draft) > s.model.dims.n_text_ctx:
                refuse(-1, "text context exceeded")
        out, record = [], []
        for s, initial, draft, sot_index, state, no_speech in windows:
            s.decode(np.asarray([initial], np.int64), first=True, sot_index=sot_index)
            nsp = float(s.no_speech_prob(no_speech)[0]) if no_speech is not None else float("nan")
            picks, st = [s.pick_greedy(**state)], state
            for t in draft:
                st = TR._next_pick_state(st, t)
                s.decode(np.asarray([[int(t)]], np.int64), first=False)
                picks.append(s.pick_greedy(**st))
            k, nxt, lp, total = TR._accept_draft(picks, draft, state["eot"], ended=initial[-1] == state["eot"])
            # left at position P0 + k through the arithmetic of the stepwise decode it stands in for (the oracle's prefill of
            # the longer prompt rounds differently, and the callers of this stand-in compare results exactly)
            s.decode(np.asarray([initial], np.int64), first=True, sot_index=sot_index)
            for t in draft[:k]:
                s.decode(np.asarray([[int(t)]], np.int64), first=False)
            res = dict(accepted=k, next_token=nxt, next_logprob=lp, sum_logprob=total, no_speech_prob=nsp)
            if want_picks:
                res["picks"] = (np.asarray([p[0] for p in picks], np.int32), np.asarray([p[1] for p in picks], np.float32))
            out.append(res)
            record.append((len(initial), len(draft), k))
        self.verifies.append(record)
        return out
