"""Shared by tests/test_gpu_window_burst.py and tests/test_window_burst_cpu.py (TEST infrastructure only), modelled on
tests/window_group_cases.py: the eight greedy windows the burst tests step, the enumeration of rule transitions both
files walk, and an oracle-backed stand-in for ``HipWindowGroup.run_pick``.

The windows are chosen so that the CPU oracle separates the best allowed token from the runner-up by >= 1e-3 in
log-probability at every step (test_window_burst_cpu.py asserts it for exactly these seeds), so the GPU comparisons are
bit for bit without a tie escape."""
import numpy as np

import window_group_cases as WG
from whisperlivekit_amd import _lib, transcribe as TR

MODEL, SEED, MARGIN = WG.MODEL, WG.SEED, WG.MARGIN

# As window_group_cases.WINDOWS (its "join" is not used here: every window opens before the first burst).  keep_eot:
# <|endoftext|> is NOT suppressed - under random weights such a window ends soon, here at its sixth step behind the
# prefill's pick, i.e. in the middle of a burst of 5 or 16 while its neighbours go on.
WINDOWS = [
    WG.WINDOWS[0],
    WG.WINDOWS[4],                                                       # without timestamps
    WG.WINDOWS[5],
    dict(seconds=5.0, seed=8, prompt="full", sample_len=20),             # ONE free position: its room is 1 inside any burst
    dict(seconds=9.0, seed=7, prompt="tile", sample_len=20),
    dict(seconds=6.5, seed=13, prompt=0, sample_len=22),                 # timestamps on, a long walk through the rules
    dict(seconds=8.5, seed=15, prompt=5, sample_len=20),
    dict(seconds=6.0, seed=30, prompt=0, sample_len=12, keep_eot=True),  # ends at <|endoftext|>, EOT_STEPS steps behind its first pick
]
EOT_WINDOW, EOT_STEPS = 7, 6              # step 6 of a burst of 16; step 1 of the second burst of 5
FULL_WINDOW = 3
# the budget (max_steps) a window hands to its FIRST burst; the others, and every later burst, hand down what is left of
# their sample_len - so budgets of 1, 2 and "the whole burst" meet in one call
FIRST_BUDGET = {1: 1, 2: 2}
# the windows of a stack of n: by budget, by <|endoftext|> mid-burst and by context room mid-burst, each beside rows that go on
STACKS = {1: [5], 2: [0, 7], 3: [3, 1, 5], 8: list(range(8))}
BURSTS = [1, 2, 3, 5, 16]
TS_WINDOWS = [0, 2, 5, 6]                 # timestamps on, <|endoftext|> suppressed: between them every ts_mode transition


class Win(WG.Win):
    def __init__(self, index, spec, model, session):
        super().__init__(index, spec, model, session)
        if spec.get("keep_eot"):
            self.dec.suppressed = [t for t in self.dec.suppressed if t != self.dec.tok.eot]

    def budget(self):
        """steps this window may still take: what is left of its sample_len"""
        return self.spec["sample_len"] - len(self.picks)


# ---- the rule transitions both files enumerate ---------------------------------------------------------------------------------
def histories(dec, rng):
    """tests/test_gpu_window_group.py's `_histories`, restated: sampled-token histories that walk every branch of
    ApplyTimestampRules."""
    tb, eot = dec.tok.timestamp_begin, dec.tok.eot
    text = lambda n: [int(t) for t in rng.integers(300, 20000, n)]
    return [[], [tb], [tb + 3], [tb, *text(3)], [tb, *text(2), tb + 40], [tb, *text(2), tb + 40, tb + 40],
            [tb, *text(1), tb + 40, tb + 40, *text(2)], [tb, *text(4), tb + 1499], [tb, *text(2), tb + 700, tb + 700, eot],
            text(5), [tb + 1500], [tb, *text(2), tb + 1500, tb + 1500]]


def state_of(dec, history):
    return dec._pick_state(np.asarray([list(dec.initial) + [int(t) for t in history]], np.int64))


def allowed(p, v):
    """rules_allowed of csrc/select.hip for one token, the suppress lists aside"""
    if p["without_timestamps"]:
        return True
    tb = p["timestamp_begin"]
    if v == p["no_timestamps"] or (p["ts_mode"] == 1 and v >= tb) or (p["ts_mode"] == 2 and v < p["eot"]):
        return False
    if tb <= v < p["ts_bound"]:
        return False
    if p["first_step"] and (v < tb or (p["max_initial"] >= 0 and v >= tb + p["max_initial"] + 1)):
        return False
    return True


def _candidates(dec, p, history, rng, n_vocab):
    """a text token, <|endoftext|>, the lowest timestamp the bound leaves, a timestamp above the bound, and the last stamp
    itself (what closes a pair)"""
    tb, eot = dec.tok.timestamp_begin, dec.tok.eot
    out = [int(rng.integers(300, 20000)), eot]
    lo = max(p["ts_bound"], tb)
    if lo < n_vocab:
        out += [lo, int(rng.integers(lo, n_vocab))]
    stamps = [t for t in history if t >= tb]
    if stamps:
        out.append(stamps[-1])
    return out


def transition_cases(model, n_walks=2000, max_len=12, seed=7):
    """-> [(decoder, history, token)]: every history of `histories` extended by each candidate the rules allow, and
    `n_walks` random walks of at most `max_len` tokens that obey the rules (every prefix with its next token), with and
    without ``without_timestamps``."""
    V = model.dims.n_vocab
    eot = TR._tokenizer_for(model, "en", "transcribe").eot
    decs = [TR._WindowDecoder(model, TR.DecodingOptions(language="en", temperature=0.0, suppress_tokens=f"-1,{eot}",
                                                        without_timestamps=flag)) for flag in (False, True)]
    rng = np.random.default_rng(seed)
    cases = []
    for dec in decs:
        for h in histories(dec, rng):
            p = state_of(dec, h)
            for t in _candidates(dec, p, h, rng, V):
                if allowed(p, t):
                    cases.append((dec, list(h), int(t)))
    for w in range(n_walks):
        dec = decs[w % 2]
        h = []
        for _ in range(int(rng.integers(1, max_len + 1))):
            p = state_of(dec, h)
            ok = [t for t in _candidates(dec, p, h, rng, V) if allowed(p, t)]
            if len(ok) > 1 and rng.random() < 0.8:           # <|endoftext|> ends a walk: let most of them run on
                ok = [t for t in ok if t != dec.tok.eot] or ok
            if not ok:
                break
            t = int(ok[int(rng.integers(len(ok)))])
            cases.append((dec, list(h), t))
            h.append(t)
            if t == dec.tok.eot:
                break
    return cases


# ---- oracle-backed stand-in ----------------------------------------------------------------------------------------------------
class OracleBurstGroup(WG.OracleGroup):
    """OracleGroup with ``run_pick``: the library's host checks first (a refused call advances nobody), then every row steps
    with the oracle for min(max_steps, burst, free positions) steps or up to <|endoftext|>, its rule state advanced by
    ``transcribe._next_pick_state``.  ``bursts``: (rows, burst, steps per row) of every call that got through."""

    def __init__(self, rows=8, break_at=None):
        super().__init__(rows, break_at)
        self.bursts = []

    def run_pick(self, sessions, tokens, states, max_steps, burst):
        call, self.n_calls = self.n_calls, self.n_calls + 1
        if call == self.break_at:
            raise RuntimeError("the device is gone")

        def refuse(code, what):
            err = _lib.WlkError(f"wlk_hip error {code}: {what}")
            err.code = code
            raise err
        if not 1 <= len(sessions) <= self.rows or len(set(map(id, sessions))) != len(sessions):
            refuse(-1, "bad rows")
        if not 1 <= burst <= 16 or any(int(m) < 1 for m in max_steps):
            refuse(-1, "bad burst")
        for s in sessions:
            if s.self_len + 1 > s.model.dims.n_text_ctx:
                refuse(-3, "text context exceeded")
        out = []
        for s, t, st, limit in zip(sessions, tokens, states, max_steps):
            ids, lps = [], []
            for _ in range(min(int(limit), burst, s.model.dims.n_text_ctx - s.self_len)):
                s.decode(np.asarray([[int(t)]], np.int64), first=False)
                t, lp = s.pick_greedy(**st)
                ids.append(t)
                lps.append(lp)
                if t == st["eot"]:
                    break
                st = TR._next_pick_state(st, t)
            out.append((np.asarray(ids, np.int32), np.asarray(lps, np.float32)))
        self.bursts.append((len(sessions), burst, [len(o[0]) for o in out]))
        self.calls.append(len(sessions))
        return out
