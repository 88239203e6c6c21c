"""Shared by tests/test_gpu_window_group.py and tests/test_window_stack_cpu.py (TEST infrastructure only): the eight greedy
windows the window-group tests step, the driver that lets them join and leave a stacked loop at different steps, the host
form of the device pick over a wlk_pick_params block, and oracle-backed stand-ins for a picking session and a window group.

The windows are chosen so that the CPU oracle separates the best allowed token from the runner-up by >= 1e-3 in
log-probability at every step (test_window_stack_cpu.py asserts it for exactly these seeds), so the GPU comparisons of
token ids need no tie escape."""
import numpy as np

from oracle_session import OracleModel, OracleSession
from whisperlivekit_amd import _lib, synth, transcribe as TR

MODEL, SEED = "micro.en", 3
MARGIN = 1e-3

# seconds / seed of synth.speech_like; prompt: carried prompt ids in front of the sot sequence ("tile": as many as make the
# prefill end exactly at a 32-row tile, "full": as many as leave ONE free position in the text context); join: the loop
# iteration at which the window's prefill happens; force_eot: the own step before which its suppress list is swapped for
# "everything but <|endoftext|>"
WINDOWS = [
    dict(seconds=7.0, seed=5, prompt=0, join=0, sample_len=12),
    dict(seconds=3.0, seed=6, prompt=40, join=0, sample_len=5),                     # leaves at sample_len
    dict(seconds=9.0, seed=7, prompt="tile", join=1, sample_len=20, force_eot=4),   # leaves at a forced <|endoftext|>
    dict(seconds=5.0, seed=8, prompt="full", join=2, sample_len=20),                # leaves at n_ctx after one stacked step
    dict(seconds=4.0, seed=9, prompt=0, join=0, sample_len=9, without_timestamps=True),
    dict(seconds=6.0, seed=10, prompt=0, join=2, sample_len=24),
    dict(seconds=8.0, seed=11, prompt=10, join=1, sample_len=16),
    dict(seconds=3.5, seed=12, prompt=3, join=2, sample_len=7),
]

# test_decode_many_equals_decode_per_window: a silent window in front of these; once as the options come (under random weights
# the windows end within a step or two), once with <|endoftext|> suppressed (every window runs to sample_len)
DECODE_MANY_WINDOWS = [WINDOWS[0], WINDOWS[1], WINDOWS[4], WINDOWS[5]]
DECODE_MANY_OPTIONS = [dict(language="en", temperature=0.0, sample_len=24),
                       dict(language="en", temperature=0.0, sample_len=12, suppress_tokens="-1,50256")]
# test_the_stacker_under_threads: transcribe() of the eight windows' recordings (no timestamps: one window per recording)
TRANSCRIBE_KW = dict(language="en", temperature=0.0, sample_len=12, suppress_tokens="-1,50256", without_timestamps=True,
                     logprob_threshold=None, compression_ratio_threshold=None, no_speech_threshold=None)
# test_one_case_on_tiny_en_dimensions: (seconds, seed) of three recordings, stacked steps behind the first pick
TINY = dict(model="tiny.en", seed=1, audios=[(3.0, 20), (5.0, 21), (7.0, 22)], steps=6)


def window_audio(spec):
    return synth.speech_like(spec["seconds"], seed=spec["seed"])


class Win:
    """One window of a drive: its decoder (rules, initial tokens), its session, its tokens so far and what it picked."""

    def __init__(self, index, spec, model, session):
        self.index, self.spec, self.session = index, spec, session
        # <|endoftext|> joins the suppress list: under random weights a greedy window would otherwise end within two steps
        eot = TR._tokenizer_for(model, "en", "transcribe").eot
        dec = TR._WindowDecoder(model, TR.DecodingOptions(language="en", temperature=0.0, sample_len=spec["sample_len"],
                                                          suppress_tokens=f"-1,{eot}",
                                                          without_timestamps=spec.get("without_timestamps", False)))
        n_ctx = model.dims.n_text_ctx
        n_prompt = spec["prompt"]
        if n_prompt == "tile":
            n_prompt = 32 - 1 - len(dec.initial)
        elif n_prompt == "full":
            n_prompt = n_ctx - 1 - 1 - len(dec.initial)
        if n_prompt:
            rng = np.random.default_rng(100 + spec["seed"])
            dec.initial = [dec.tok.sot_prev] + [int(t) for t in rng.integers(300, 20000, n_prompt)] + list(dec.initial)
            dec.sample_begin = len(dec.initial)
            dec.sot_index = dec.initial.index(dec.tok.sot)
        self.dec = dec
        self.tokens = np.asarray([dec.initial], np.int64)
        self.sum_logprobs = np.zeros(1, np.float32)
        self.picks = []                  # (token, log-probability) per own step, the prefill's pick first
        self.extra = []                  # what the backend wants to keep per own step (logits, margins)
        self.over = False

    def rules(self):
        return self.dec.suppressed or [], self.dec.blank_ids or []

    def eot_only_rules(self, n_vocab):
        """the suppress list that leaves <|endoftext|> alone"""
        return [t for t in range(n_vocab) if t != self.dec.tok.eot], []

    def take(self, tok, lp, extra=None):
        self.picks.append((int(tok), float(lp)))
        self.extra.append(extra)
        self.tokens, over = TR._greedy_take(self.tokens, self.sum_logprobs, int(tok), float(lp), self.dec.tok.eot,
                                            self.dec.n_ctx)
        self.over = over or len(self.picks) >= self.spec["sample_len"]


def drive(wins, open_window, step, force_eot):
    """Runs `wins` to their ends: at iteration g the windows with join == g are opened (``open_window(w)`` -> (token,
    log-probability, extra) of the prefill's own pick), then every window in flight takes one step (``step(list)`` -> one
    such triple per window).  ``force_eot(w)`` swaps w's suppress list before the step its spec names."""
    pending = sorted(wins, key=lambda w: w.spec["join"])
    live, g, group_sizes = [], 0, []
    while pending or live:
        while pending and pending[0].spec["join"] <= g:
            w = pending.pop(0)
            w.take(*open_window(w))
            if not w.over:
                live.append(w)
        if live:
            for w in live:
                if w.spec.get("force_eot") == len(w.picks):
                    force_eot(w)
            group_sizes.append(len(live))
            for w, res in zip(list(live), step(list(live))):
                w.take(*res)
            live = [w for w in live if not w.over]
        g += 1
        assert g < 200
    return group_sizes


# ---- the host form of the device pick -----------------------------------------------------------------------------------------
def allowed_by_pick_params(p, suppressed, blank, n_vocab):
    """rules_allowed of csrc/select.hip over the wlk_pick_params fields (the form tests/test_transcribe.py pins against
    `_apply_rules`)."""
    v = np.arange(n_vocab)
    ok = np.ones(n_vocab, bool)
    ok[list(suppressed)] = False
    if p["first_step"]:
        ok[list(blank)] = False
    if p["without_timestamps"]:
        return ok
    tb = p["timestamp_begin"]
    if p["no_timestamps"] >= 0:
        ok[p["no_timestamps"]] = False
    if p["ts_mode"] == 1:
        ok &= v < tb
    if p["ts_mode"] == 2:
        ok &= v >= p["eot"]
    ok &= ~((v >= tb) & (v < p["ts_bound"]))
    if p["first_step"]:
        ok &= v >= tb
        if p["max_initial"] >= 0:
            ok &= v < tb + p["max_initial"] + 1
    return ok


def host_pick(logits, p, suppressed, blank):
    """-> (token, log-probability, margin): the greedy pick under the rules in float64, and how far the decision is from
    flipping - the log-probability gap between the best and the second best allowed token, and the gap of the
    "timestamps outweigh text" comparison when both sides exist."""
    x = np.asarray(logits, np.float64).copy()
    ok = allowed_by_pick_params(p, suppressed, blank, x.size)
    x[~ok] = -np.inf

    def lsm(a):
        m = a.max()
        return a - (m + np.log(np.exp(a - m).sum()))
    lp = lsm(x)
    margin = np.inf
    tb = p["timestamp_begin"]
    if not p["without_timestamps"] and np.isfinite(lp[tb:]).any():
        ts = lp[tb:][np.isfinite(lp[tb:])]
        lse_ts = ts.max() + np.log(np.exp(ts - ts.max()).sum())
        text = lp[:tb].max()
        if np.isfinite(text):
            margin = abs(lse_ts - text)
        if lse_ts > text:
            x[:tb] = -np.inf
            lp = lsm(x)
    order = np.argsort(-lp, kind="stable")[:2]
    if np.isfinite(lp[order[1]]):
        margin = min(margin, float(lp[order[0]] - lp[order[1]]))
    return int(order[0]), float(lp[order[0]]), float(margin)


def rules_mask(n_vocab, suppressed, blank):
    """the mask wlk_rules_set builds: bit 0 = always suppressed, bit 1 = blank"""
    m = np.zeros(n_vocab, np.uint8)
    m[list(suppressed)] |= 1
    m[list(blank)] |= 2
    return m


# ---- oracle-backed stand-ins --------------------------------------------------------------------------------------------------
class PickingOracleSession(OracleSession):
    """OracleSession with the device-rules methods of HipSession (set_rules / pick_greedy), answered by `host_pick`, and
    the text-context bound of the library."""

    def __init__(self, model, beam):
        super().__init__(model, beam)
        self.suppressed, self.blank = [], []
        self.self_len = 0
        self.margins = []

    def set_rules(self, suppressed, blank):
        self.suppressed, self.blank = list(suppressed), list(blank)

    def decode(self, tokens, first, sot_index=0):
        n = np.asarray(tokens).shape[1]
        if (0 if first else self.self_len) + n > self.model.dims.n_text_ctx:
            err = _lib.WlkError("wlk_hip error -3: text context exceeded")
            err.code = -3
            raise err
        super().decode(tokens, first, sot_index)
        self.self_len = (0 if first else self.self_len) + n

    def pick_greedy(self, **p):
        tok, lp, margin = host_pick(self.logits_last[0].numpy(), p, self.suppressed, self.blank)
        self.margins.append(margin)
        return tok, lp


class PickingOracleModel(OracleModel):
    def new_session(self, beam=1, max_audio_seconds=64.0, batched=None):
        return PickingOracleSession(self, beam)


class OracleGroup:
    """Stands in for engine.HipWindowGroup: steps every row with the oracle, after the library's host checks (a refused call
    advances nobody).  ``break_at``: the step_pick call (0-based) that dies like a device failure."""

    def __init__(self, rows=8, break_at=None):
        self.rows, self.break_at = rows, break_at
        self.calls = []                  # rows per step_pick call that got through the checks
        self.n_calls = 0
        self.closed = False

    def step_pick(self, sessions, tokens, states):
        call, self.n_calls = self.n_calls, self.n_calls + 1
        if call == self.break_at:
            raise RuntimeError("the device is gone")
        if not 1 <= len(sessions) <= self.rows or len(set(map(id, sessions))) != len(sessions):
            err = _lib.WlkError("wlk_hip error -1: bad rows")
            err.code = -1
            raise err
        for s in sessions:
            if s.self_len + 1 > s.model.dims.n_text_ctx:
                err = _lib.WlkError("wlk_hip error -3: text context exceeded")
                err.code = -3
                raise err
        self.calls.append(len(sessions))
        out = []
        for s, t, st in zip(sessions, tokens, states):
            s.decode(np.asarray([[int(t)]], np.int64), first=False)
            out.append(s.pick_greedy(**st))
        return np.asarray([o[0] for o in out], np.int32), np.asarray([o[1] for o in out], np.float32)

    def stats(self):
        steps, rows = len(self.calls), sum(self.calls)
        return dict(steps=steps, rows=rows, mean_rows_per_step=round(rows / steps, 3) if steps else None)

    def close(self):
        self.closed = True
