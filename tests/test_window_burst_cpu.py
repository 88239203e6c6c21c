"""The host half of bursts of greedy steps (whisperlivekit_amd/transcribe.py: _next_pick_state, WindowStacker(burst=k), the
switch) over oracle-backed stand-ins (tests/window_burst_cases.py), and the decision margins of the windows the GPU tests
step (tests/test_gpu_window_burst.py)."""
import threading

import numpy as np
import pytest

import helpers as H
import window_burst_cases as WB
import window_group_cases as WG
from whisperlivekit_amd import synth, transcribe as TR


@pytest.fixture()
def real_vocab(tmp_path, monkeypatch):
    monkeypatch.setenv("WLK_VOCAB_DIR", H.real_vocab_dir(tmp_path))
    monkeypatch.setenv("WLK_SYNTHETIC_VOCAB", "0")
    monkeypatch.delenv("WLK_TRANSCRIBE_STACK", raising=False)
    monkeypatch.delenv("WLK_TRANSCRIBE_STACK_BURST", raising=False)


@pytest.fixture()
def model():
    return WG.PickingOracleModel(WG.MODEL, WG.SEED)


OPTS = dict(language="en", temperature=0.0, sample_len=10)


def _mel(model, seconds, seed):
    s = model.new_session()
    return TR.pad_or_trim(s.log_mel(synth.speech_like(seconds, seed=seed)))


# ---- 1. the rule transition ---------------------------------------------------------------------------------------------------
def test_the_next_rule_state_is_the_state_of_the_longer_history(real_vocab, model):
    """_next_pick_state(_pick_state(h), t) == _pick_state(h + [t]) over the histories of the rule tests extended by every
    kind of token the rules allow, and over 2 000 random walks that obey the rules, with and without timestamps."""
    cases = WB.transition_cases(model)
    seen = set()
    for dec, h, t in cases:
        before = WB.state_of(dec, h)
        assert WB.allowed(before, t)
        got, want = TR._next_pick_state(before, t), WB.state_of(dec, h + [t])
        assert got == want, (h, t, before, got, want)
        seen.add((bool(before["first_step"]), bool(before["without_timestamps"]), before["ts_mode"], want["ts_mode"]))
    # every mode change with timestamps on (0 -> 1 only as the first step), a closed pair repeated at the last stamp, and
    # the same walk of ts_mode with the rules off (it is derived from the history either way)
    assert {(True, False, 0, 1), (False, False, 1, 0), (False, False, 0, 2), (False, False, 2, 1), (False, False, 0, 0),
            (False, False, 2, 0)} <= seen, seen
    assert any(wt for _f, wt, _a, _b in seen)
    assert any(t == [x for x in h if x >= dec.tok.timestamp_begin][-1] for dec, h, t in cases
               if t >= dec.tok.timestamp_begin and any(x >= dec.tok.timestamp_begin for x in h))
    assert any(t == dec.tok.eot for dec, _h, t in cases)
    assert len(cases) > 2000 + 2 * 12 and max(len(h) for _d, h, _t in cases) == 11


# ---- 2. the GPU tests' windows ------------------------------------------------------------------------------------------------
def test_the_burst_windows_keep_their_decisions_clear_of_rounding(real_vocab, model):
    """At every step of the eight windows of tests/window_burst_cases.py the oracle's best allowed token leads the runner-up
    by >= 1e-3 in log-probability - the <|endoftext|> pick included - so the GPU file compares bits without a tie escape;
    the windows end the way that file relies on, and the timestamped ones walk every change of ts_mode."""
    wins, walked = [], set()
    for i, spec in enumerate(WB.WINDOWS):
        w = WB.Win(i, spec, model, model.new_session())
        s = w.session
        s.encode_mel(TR.pad_or_trim(s.log_mel(WG.window_audio(spec))))
        s.set_rules(*w.rules())
        s.decode(w.tokens, first=True, sot_index=w.dec.sot_index)
        state = w.dec._pick_state(w.tokens)
        w.take(*s.pick_greedy(**state), s.margins[-1])
        while not w.over:
            nxt = TR._next_pick_state(state, w.picks[-1][0])
            assert nxt == w.dec._pick_state(w.tokens)
            if i in WB.TS_WINDOWS:
                walked.add((state["ts_mode"], nxt["ts_mode"]))
            state = nxt
            s.decode(w.tokens[:, -1:], first=False)
            w.take(*s.pick_greedy(**state), s.margins[-1])
        wins.append(w)
    print("steps per window:", [len(w.picks) for w in wins], f"worst margin {min(m for w in wins for m in w.extra):.3e}")
    for w in wins:
        assert min(w.extra) >= WB.MARGIN, (w.index, [f"{m:.2e}" for m in w.extra])
    assert {(0, 1), (1, 0), (0, 2), (2, 1)} <= walked, walked
    eot = wins[0].dec.tok.eot
    e = wins[WB.EOT_WINDOW]
    assert e.picks[-1][0] == eot and len(e.picks) == 1 + WB.EOT_STEPS < e.spec["sample_len"]
    assert all(w.picks[-1][0] != eot for w in wins if w is not e)
    f = wins[WB.FULL_WINDOW]
    assert len(f.picks) == 2 and f.tokens.shape[1] == model.dims.n_text_ctx + 1              # ONE step behind its first pick
    assert all(len(w.picks) == w.spec["sample_len"] for w in wins if w is not e and w is not f)
    assert all(wins[i].spec["sample_len"] >= 20 and not wins[i].spec.get("without_timestamps") for i in (5, 6))


# ---- 3. the stacker -----------------------------------------------------------------------------------------------------------
def test_the_switch_argument_wins_over_the_environment_and_the_range_is_checked(monkeypatch):
    monkeypatch.delenv("WLK_TRANSCRIBE_STACK_BURST", raising=False)
    assert TR.resolve_burst(None) == 1
    monkeypatch.setenv("WLK_TRANSCRIBE_STACK_BURST", "5")
    assert TR.resolve_burst(None) == 5 and TR.resolve_burst(1) == 1 and TR.resolve_burst(16) == 16
    for bad in (0, 17, -3):
        with pytest.raises(ValueError):
            TR.resolve_burst(bad)
        with pytest.raises(ValueError):
            TR.WindowStacker(None, 8, group=WB.OracleBurstGroup(8), burst=bad)
    assert TR.WindowStacker(None, 8, group=WB.OracleBurstGroup(8)).burst == 5
    assert TR.WindowStacker(None, 8, group=WB.OracleBurstGroup(8), burst=2).burst == 2
    monkeypatch.setenv("WLK_TRANSCRIBE_STACK_BURST", "17")
    with pytest.raises(ValueError):
        TR.resolve_burst(None)

    class M:
        pass
    m = M()
    monkeypatch.setenv("WLK_TRANSCRIBE_STACK_BURST", "4")
    monkeypatch.setenv("WLK_TRANSCRIBE_STACK", "3")
    real = TR.WindowStacker
    monkeypatch.setattr(TR, "WindowStacker", lambda model, rows: real(model, rows, group=WB.OracleBurstGroup(rows)))
    assert TR._run_stacker(m).burst == 4
    assert TR.set_burst(m, 1) == 1 and TR._run_stacker(m).burst == 1           # an explicit 1 switches the environment's 4 off
    assert TR.set_burst(m, 9) == 9 and TR._run_stacker(m).burst == 9
    assert TR.set_burst(m, None) == 4 and TR._run_stacker(m).burst == 4
    with pytest.raises(ValueError):
        TR.set_burst(m, 0)


def test_the_asr_front_takes_burst_and_needs_a_stack(monkeypatch):
    from whisperlivekit_amd.local_agreement import HipWhisperASR
    monkeypatch.delenv("WLK_TRANSCRIBE_STACK", raising=False)
    monkeypatch.delenv("WLK_TRANSCRIBE_STACK_BURST", raising=False)

    class M:
        pass
    m = M()
    asr = HipWhisperASR("en", hip_model=m, stack=4, burst=8)
    assert (asr.stack, asr.burst) == (4, 8) and m.__dict__["_window_stack_burst"] == 8
    assert HipWhisperASR("en", hip_model=M()).burst == 1
    with pytest.raises(ValueError):
        HipWhisperASR("en", hip_model=M(), burst=4)            # needs stack >= 1
    with pytest.raises(ValueError):
        HipWhisperASR("en", hip_model=M(), stack=2, burst=17)


def test_with_burst_one_run_pick_is_never_called_and_nothing_new_is_constructed(real_vocab, model, monkeypatch):
    class NoRunPick(WG.OracleGroup):
        def run_pick(self, *a, **k):
            raise AssertionError("run_pick although the burst is 1")
    mels = [_mel(model, 7.0, 5), _mel(model, 3.0, 6)]
    opts = TR.DecodingOptions(**OPTS)
    want = [TR.decode(model, m, opts) for m in mels]
    group = NoRunPick(8)
    stacker = TR.WindowStacker(model, 8, group=group, solo_single=False)
    assert stacker.burst == 1
    assert TR.decode_many(model, mels, opts, stacker=stacker) == want and group.calls
    # switched off altogether, a burst in the environment constructs nothing
    from whisperlivekit_amd import engine

    def never(*a, **k):
        raise AssertionError("constructed although stacking is off")
    monkeypatch.setenv("WLK_TRANSCRIBE_STACK_BURST", "8")
    monkeypatch.setattr(TR, "WindowStacker", never)
    monkeypatch.setattr(engine, "HipWindowGroup", never)
    assert TR.decode(model, mels[0], opts) == want[0] and "_window_stacker" not in model.__dict__
    TR.release_sessions(model)


@pytest.mark.parametrize("burst", [1, 2, 5, 16])
def test_bursts_give_the_tokens_and_sums_of_single_steps(burst, real_vocab, model):
    """decode_many through WindowStacker(burst=k) against decode() per window: same tokens, same sums; the calls are as long
    as the longest budget allows and no longer."""
    mels = [_mel(model, 4.0, 9), np.zeros((80, 3000), np.float32), _mel(model, 7.0, 5), _mel(model, 3.0, 6)]
    for opts in (TR.DecodingOptions(**OPTS), TR.DecodingOptions(**dict(OPTS, sample_len=12, suppress_tokens="-1,50256"))):
        want = [TR.decode(model, m, opts) for m in mels]
        group = WB.OracleBurstGroup(8)
        got = TR.decode_many(model, mels, opts, stacker=TR.WindowStacker(model, 8, group=group, solo_single=False, burst=burst))
        assert [g.tokens for g in got] == [w.tokens for w in want]
        for g, w in zip(got, want):
            assert (g.text, g.no_speech_prob, g.avg_logprob, g.compression_ratio) == \
                (w.text, w.no_speech_prob, w.avg_logprob, w.compression_ratio)
        own = sum(min(len(w.tokens) + 1, opts.sample_len) - 1 for w in want)
        if burst == 1:
            assert not group.bursts and sum(group.calls) == own
        else:
            assert sum(sum(steps) for _n, _k, steps in group.bursts) == own
            assert all(k <= burst and max(steps) <= k for _n, k, steps in group.bursts)
    TR.release_sessions(model)


class GatedBurstGroup(WB.OracleBurstGroup):
    """lets a test hold the runner inside a burst while other threads queue their windows"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.entered = threading.Event()
        self.go = threading.Event()

    def run_pick(self, *a):
        if self.n_calls == 0:
            self.entered.set()
            assert self.go.wait(60)
        return super().run_pick(*a)


def _window(model, seconds, seed, sample_len=10):
    dec = TR._WindowDecoder(model, TR.DecodingOptions(**dict(OPTS, sample_len=sample_len, suppress_tokens="-1,50256")))
    got = dec.run(_mel(model, seconds, seed), model.new_session(), stacker=object(), defer=True)
    assert isinstance(got, tuple)
    return got


def _threads(stacker, windows):
    errors = [None] * len(windows)

    def work(i):
        try:
            stacker.run(windows[i])
        except BaseException as e:
            errors[i] = e
    return [threading.Thread(target=work, args=(i,)) for i in range(len(windows))], errors


def _join_all(ts):
    for t in ts:
        t.join(60)
    assert not any(t.is_alive() for t in ts), "a waiter is still blocked"


def test_a_window_queued_during_a_burst_rides_the_next_one(real_vocab, model):
    opts = TR.DecodingOptions(**dict(OPTS, suppress_tokens="-1,50256"))
    specs = [(7.0, 5), (3.0, 6), (4.0, 9)]
    want = [TR.decode(model, _mel(model, *sp), opts) for sp in specs]
    group = GatedBurstGroup(8)
    stacker = TR.WindowStacker(model, 8, group=group, solo_single=False, burst=4)
    made = [_window(model, *sp) for sp in specs]
    ts, errors = _threads(stacker, [w for w, _f in made])
    ts[0].start()
    assert group.entered.wait(60)                      # the first caller is the runner and sits in its first burst
    ts[1].start(); ts[2].start()
    while True:
        with stacker._cv:
            if len(stacker._queue) == 2:
                break
    group.go.set()
    _join_all(ts)
    assert errors == [None] * 3
    # 9 steps each: the first window alone for 4, then all three - the late ones still have 9 to go, the first one 5
    assert group.bursts[0] == (1, 4, [4]) and group.bursts[1] == (3, 4, [4, 4, 4]), group.bursts
    assert group.bursts[2] == (3, 4, [1, 4, 4]) and group.bursts[3] == (2, 1, [1, 1]), group.bursts
    assert [f().tokens for _w, f in made] == [w.tokens for w in want]
    assert stacker.passes == 1 and stacker.stats()["windows"] == 3
    TR.release_sessions(model)


def test_a_refused_window_fails_alone_in_a_burst(real_vocab, model):
    opts = TR.DecodingOptions(**dict(OPTS, suppress_tokens="-1,50256"))
    want = TR.decode(model, _mel(model, 7.0, 5), opts)
    good, finish = _window(model, 7.0, 5)
    full, _f = _window(model, 3.0, 6)
    full.session.self_len = model.dims.n_text_ctx      # context full
    group = WB.OracleBurstGroup(8)
    stacker = TR.WindowStacker(model, 8, group=group, solo_single=False, burst=5)
    ts, errors = _threads(stacker, [good, full])
    for t in ts:
        t.start()
    _join_all(ts)
    assert errors[0] is None and getattr(errors[1], "code", None) == -3, errors
    assert finish().tokens == want.tokens and finish().avg_logprob == want.avg_logprob
    assert all(n == 1 for n, _k, _s in group.bursts)   # the refused call advanced nobody; from then on the good one alone
    TR.release_sessions(model)


def test_a_broken_burst_reaches_everyone(real_vocab, model):
    group = WB.OracleBurstGroup(8, break_at=1)
    stacker = TR.WindowStacker(model, 8, group=group, solo_single=False, burst=3)
    made = [_window(model, *sp) for sp in [(7.0, 5), (3.0, 6)]]
    with pytest.raises(RuntimeError, match="device is gone"):
        stacker.run_many([w for w, _f in made])
    assert len(group.bursts) == 1 and not stacker._running and not stacker._open and not stacker._queue
    late, finish = _window(model, 4.0, 9)
    stacker.run(late)                                  # the next caller starts a fresh pass
    assert stacker.passes == 2 and len(finish().tokens) > 0


def test_a_lone_window_keeps_its_own_chain_with_bursts_on(real_vocab, model):
    opts = TR.DecodingOptions(**OPTS)
    mel = _mel(model, 7.0, 5)
    want = TR.decode(model, mel, opts)
    group = WB.OracleBurstGroup(8)
    stacker = TR.WindowStacker(model, 8, group=group, burst=8)
    assert TR.decode_many(model, [mel], opts, stacker=stacker)[0] == want
    assert group.n_calls == 0 and stacker.solo_steps == min(len(want.tokens) + 1, OPTS["sample_len"]) - 1
    TR.release_sessions(model)
