"""The host half of the stacked greedy windows (whisperlivekit_amd/transcribe.py: decode_many, WindowStacker, the switch)
over oracle-backed stand-in sessions and a stand-in window group (tests/window_group_cases.py), and the decision margins
of the windows the GPU tests step (tests/test_gpu_window_group.py)."""
import threading

import numpy as np
import pytest

import helpers as H
import window_group_cases as WG
from whisperlivekit_amd import synth, transcribe as TR


@pytest.fixture()
def real_vocab(tmp_path, monkeypatch):
    monkeypatch.setenv("WLK_VOCAB_DIR", H.real_vocab_dir(tmp_path))
    monkeypatch.setenv("WLK_SYNTHETIC_VOCAB", "0")
    monkeypatch.delenv("WLK_TRANSCRIBE_STACK", raising=False)


def _mel(model, seconds, seed):
    s = model.new_session()
    return TR.pad_or_trim(s.log_mel(synth.speech_like(seconds, seed=seed)))


OPTS = dict(language="en", temperature=0.0, sample_len=10)


@pytest.fixture()
def model():
    return WG.PickingOracleModel(WG.MODEL, WG.SEED)


def test_switch_argument_wins_over_the_environment_and_the_range_is_checked(monkeypatch):
    monkeypatch.delenv("WLK_TRANSCRIBE_STACK", raising=False)
    assert TR.resolve_stack(None) == 0
    monkeypatch.setenv("WLK_TRANSCRIBE_STACK", "5")
    assert TR.resolve_stack(None) == 5
    assert TR.resolve_stack(0) == 0 and TR.resolve_stack(8) == 8
    for bad in (-1, 9):
        with pytest.raises(ValueError):
            TR.resolve_stack(bad)
    monkeypatch.setenv("WLK_TRANSCRIBE_STACK", "9")
    with pytest.raises(ValueError):
        TR.resolve_stack(None)

    class M:
        pass
    m = M()
    monkeypatch.setenv("WLK_TRANSCRIBE_STACK", "4")
    assert TR.set_stack(m, 0) == 0 and TR._run_stacker(m) is None          # an explicit 0 switches the environment's 4 off
    monkeypatch.setattr(TR, "WindowStacker", lambda model, rows: ("stacker", rows))
    assert TR.set_stack(m, None) == 4 and TR._run_stacker(m) == ("stacker", 4)


def test_switch_off_constructs_neither_stacker_nor_group(real_vocab, model, monkeypatch):
    from whisperlivekit_amd import engine

    def never(*a, **k):
        raise AssertionError("constructed although stacking is off")
    monkeypatch.setattr(TR, "WindowStacker", never)
    monkeypatch.setattr(engine, "HipWindowGroup", never)
    got = TR.decode(model, _mel(model, 4.0, 9), TR.DecodingOptions(**OPTS))
    assert len(got.tokens) > 0 and "_window_stacker" not in model.__dict__
    TR.release_sessions(model)


def test_decode_many_equals_decode_per_window_and_rows_leave_alone(real_vocab, model):
    mels = [_mel(model, 4.0, 9), np.zeros((80, 3000), np.float32), _mel(model, 7.0, 5), _mel(model, 3.0, 6)]
    opts = TR.DecodingOptions(**OPTS)
    want = [TR.decode(model, m, opts) for m in mels]
    group = WG.OracleGroup(8)
    got = TR.decode_many(model, mels, opts, stacker=TR.WindowStacker(model, 8, group=group, solo_single=False))
    assert [g.tokens for g in got] == [w.tokens for w in want]
    for g, w in zip(got, want):
        assert (g.text, g.no_speech_prob, g.temperature, g.language) == (w.text, w.no_speech_prob, w.temperature, w.language)
        assert g.avg_logprob == w.avg_logprob and g.compression_ratio == w.compression_ratio
    # every window took its own steps and no more: the calls shrink as windows end
    assert sum(group.calls) == sum(min(len(w.tokens) + 1, OPTS["sample_len"]) - 1 for w in want)
    assert group.calls[0] == len(mels) and group.calls == sorted(group.calls, reverse=True)
    with pytest.raises(ValueError):
        TR.decode_many(model, mels, opts, temperature=0.2)
    TR.release_sessions(model)


class GatedGroup(WG.OracleGroup):
    """lets a test hold the runner inside a step while other threads queue their windows"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.entered = threading.Event()
        self.go = threading.Event()
        self.hold_call = 0

    def step_pick(self, sessions, tokens, states):
        if self.n_calls == self.hold_call:
            self.entered.set()
            assert self.go.wait(60)
        return super().step_pick(sessions, tokens, states)


def _window(model, seconds, seed, sample_len=10):
    """-> (window, finish) of a greedy window behind its first pick"""
    dec = TR._WindowDecoder(model, TR.DecodingOptions(**dict(OPTS, sample_len=sample_len)))
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
    ts = [threading.Thread(target=work, args=(i,)) for i in range(len(windows))]
    return ts, errors


def _join_all(ts):
    for t in ts:
        t.join(60)
    assert not any(t.is_alive() for t in ts), "a waiter is still blocked"


def test_windows_arriving_during_a_pass_are_admitted_at_its_next_step(real_vocab, model):
    opts = TR.DecodingOptions(**OPTS)
    specs = [(7.0, 5), (3.0, 6), (4.0, 9)]
    want = [TR.decode(model, _mel(model, *sp), opts) for sp in specs]
    group = GatedGroup(8)
    stacker = TR.WindowStacker(model, 8, group=group, solo_single=False)
    made = [_window(model, *sp) for sp in specs]
    ts, errors = _threads(stacker, [w for w, _f in made])
    ts[0].start()
    assert group.entered.wait(60)                      # the first caller is the runner and sits in its first step
    ts[1].start(); ts[2].start()
    while True:                                        # both others have queued (they cannot run: a pass is running)
        with stacker._cv:
            if len(stacker._queue) == 2:
                break
    group.go.set()
    _join_all(ts)
    assert errors == [None] * 3
    assert group.calls[0] == 1 and group.calls[1] == 3, group.calls
    assert [f().tokens for _w, f in made] == [w.tokens for w in want]
    assert stacker.passes == 1 and stacker.stats()["windows"] == 3
    TR.release_sessions(model)


def test_more_windows_than_rows_wait_for_a_free_row(real_vocab, model):
    specs = [(7.0, 5), (3.0, 6), (4.0, 9)]
    group = WG.OracleGroup(2)
    stacker = TR.WindowStacker(model, 2, group=group, solo_single=False)
    made = [_window(model, *sp, sample_len=4 + i) for i, sp in enumerate(specs)]
    stacker.run_many([w for w, _f in made])
    assert max(group.calls) == 2 and sum(group.calls) == sum(len(w.tokens[0]) - w.decoder.sample_begin - 1 for w, _f in made)
    assert all(len(f().tokens) > 0 for _w, f in made)


def test_a_failed_pass_reaches_every_window_and_the_next_caller_starts_fresh(real_vocab, model):
    specs = [(7.0, 5), (3.0, 6), (4.0, 9)]
    group = GatedGroup(8, break_at=1)
    stacker = TR.WindowStacker(model, 8, group=group, solo_single=False)
    made = [_window(model, *sp) for sp in specs]
    ts, errors = _threads(stacker, [w for w, _f in made])
    ts[0].start()
    assert group.entered.wait(60)
    ts[1].start()
    while True:
        with stacker._cv:
            if len(stacker._queue) == 1:
                break
    group.go.set()                                     # call 0 goes through, call 1 (both windows in flight) dies
    _join_all(ts[:2])
    assert all(isinstance(e, RuntimeError) and "device is gone" in str(e) for e in errors[:2]), errors
    assert stacker.passes == 1 and not stacker._running and not stacker._open and not stacker._queue
    ts[2].start()                                      # the next caller becomes the runner of a fresh pass
    _join_all(ts[2:])
    assert errors[2] is None and stacker.passes == 2
    assert len(made[2][1]().tokens) > 0


def test_a_refused_window_fails_alone(real_vocab, model):
    """A window whose session is at the end of its text context is refused by the group's host checks: it raises in its
    own thread, the windows stacked with it go on to the result they have alone."""
    opts = TR.DecodingOptions(**OPTS)
    want = TR.decode(model, _mel(model, 7.0, 5), opts)
    good, finish = _window(model, 7.0, 5)
    full, _f = _window(model, 3.0, 6)
    full.session.self_len = model.dims.n_text_ctx      # context full
    stacker = TR.WindowStacker(model, 8, group=WG.OracleGroup(8), solo_single=False)
    ts, errors = _threads(stacker, [good, full])
    for t in ts:
        t.start()
    _join_all(ts)
    assert errors[0] is None and getattr(errors[1], "code", None) == -3, errors
    assert finish().tokens == want.tokens and finish().avg_logprob == want.avg_logprob
    TR.release_sessions(model)


def test_run_goes_through_the_models_stacker_when_switched_on(real_vocab, model, monkeypatch):
    opts = TR.DecodingOptions(**OPTS)
    mel = _mel(model, 7.0, 5)
    want = TR.decode(model, mel, opts)
    group = WG.OracleGroup(8)
    made = []
    real = TR.WindowStacker
    monkeypatch.setattr(TR, "WindowStacker", lambda m, rows: made.append(rows) or real(m, rows, group=group, solo_single=False))
    monkeypatch.setenv("WLK_TRANSCRIBE_STACK", "3")
    got = TR.decode(model, mel, opts)
    assert made == [3] and got == want
    assert group.calls == [1] * (min(len(want.tokens) + 1, OPTS["sample_len"]) - 1)
    # sampling and the host rules never reach it
    n = group.n_calls
    monkeypatch.setenv("WLK_TRANSCRIBE_DEVICE_RULES", "0")
    assert TR.decode(model, mel, opts).tokens == want.tokens and group.n_calls == n
    TR.release_sessions(model)


def test_a_single_window_in_flight_takes_the_sessions_own_step(real_vocab, model):
    """The default front: one window in flight steps on its own chain (no group call), two or more share group steps, and
    the result is decode()'s either way."""
    opts = TR.DecodingOptions(**OPTS)
    mels = [_mel(model, 7.0, 5), _mel(model, 3.0, 6)]
    want = [TR.decode(model, m, opts) for m in mels]
    group = WG.OracleGroup(8)
    stacker = TR.WindowStacker(model, 8, group=group)
    assert TR.decode_many(model, mels[:1], opts, stacker=stacker)[0] == want[0]
    assert group.calls == [] and stacker.solo_steps == min(len(want[0].tokens) + 1, OPTS["sample_len"]) - 1
    assert TR.decode_many(model, mels, opts, stacker=stacker) == want
    assert group.calls and set(group.calls) == {2}
    full, _f = _window(model, 3.0, 6)
    full.session.self_len = model.dims.n_text_ctx      # context full: the window's own step refuses it
    with pytest.raises(Exception) as e:
        stacker.run(full)
    assert e.value.code == -3 and not stacker._running and not stacker._open
    TR.release_sessions(model)


def test_the_gpu_tests_windows_keep_their_decisions_clear_of_rounding(real_vocab):
    """Contract 4: at every step of every window of tests/window_group_cases.py the oracle's best allowed token leads the
    runner-up by >= 1e-3 in log-probability (and the "timestamps outweigh text" comparison is as far from flipping), so
    the GPU comparisons of token ids need no tie escape."""
    model = WG.PickingOracleModel(WG.MODEL, WG.SEED)
    V = model.dims.n_vocab
    wins = [WG.Win(i, spec, model, model.new_session()) for i, spec in enumerate(WG.WINDOWS)]

    def open_window(w):
        s = w.session
        s.encode_mel(TR.pad_or_trim(s.log_mel(WG.window_audio(w.spec))))
        s.set_rules(*w.rules())
        s.decode(w.tokens, first=True, sot_index=w.dec.sot_index)
        return (*s.pick_greedy(**w.dec._pick_state(w.tokens)), s.margins[-1])

    def step(live):
        out = []
        for w in live:
            w.session.decode(w.tokens[:, -1:], first=False)
            out.append((*w.session.pick_greedy(**w.dec._pick_state(w.tokens)), w.session.margins[-1]))
        return out

    sizes = WG.drive(wins, open_window, step, lambda w: w.session.set_rules(*w.eot_only_rules(V)))
    worst = min(m for w in wins for m in w.extra)
    print("steps per window:", [len(w.picks) for w in wins], "rows per step:", sizes, f"worst margin {worst:.3e}")
    for w in wins:
        assert min(w.extra) >= WG.MARGIN, (w.index, [f"{m:.2e}" for m in w.extra])
    # the schedule does what the GPU test relies on: windows join and leave at different steps, one by each kind of end
    assert max(sizes) == 8 and len(set(sizes)) > 3
    assert wins[1].picks[-1][0] != wins[1].dec.tok.eot and len(wins[1].picks) == 5          # sample_len
    assert wins[2].picks[-1][0] == wins[2].dec.tok.eot and len(wins[2].picks) == 5          # forced <|endoftext|>
    assert len(wins[3].picks) == 2 and wins[3].tokens.shape[1] == model.dims.n_text_ctx + 1  # n_ctx


def test_the_other_gpu_windows_keep_their_decisions_clear_of_rounding(real_vocab):
    """Contract 4 for the windows of the GPU file's decode_many, thread and tiny.en tests."""
    model = WG.PickingOracleModel(WG.MODEL, WG.SEED)
    s = model.new_session()
    worst = np.inf
    for opts in WG.DECODE_MANY_OPTIONS:
        mels = [np.zeros((80, 3000), np.float32)] + [TR.pad_or_trim(s.log_mel(WG.window_audio(sp))) for sp in WG.DECODE_MANY_WINDOWS]
        for mel in mels:
            s.margins = []
            TR.decode(model, mel, TR.DecodingOptions(**opts), session=s)
            assert len(s.margins) >= 1 and min(s.margins) >= WG.MARGIN, (opts, [f"{m:.2e}" for m in s.margins])
            worst = min(worst, min(s.margins))
    for sp in WG.WINDOWS:
        own = TR._rows_of(model).get(1)
        own.margins = []
        got = TR.transcribe(model, WG.window_audio(sp), **WG.TRANSCRIBE_KW)
        assert len(got["segments"]) == 1 and len(own.margins) == WG.TRANSCRIBE_KW["sample_len"]
        assert min(own.margins) >= WG.MARGIN, (sp, [f"{m:.2e}" for m in own.margins])
        worst = min(worst, min(own.margins))
    TR.release_sessions(model)
    tiny = WG.PickingOracleModel(WG.TINY["model"], WG.TINY["seed"])
    eot = TR._tokenizer_for(tiny, "en", "transcribe").eot
    assert eot == 50256
    dec = TR._WindowDecoder(tiny, TR.DecodingOptions(language="en", temperature=0.0, suppress_tokens=f"-1,{eot}"))
    for seconds, seed in WG.TINY["audios"]:
        t = tiny.new_session()
        t.encode_mel(TR.pad_or_trim(t.log_mel(synth.speech_like(seconds, seed=seed))))
        t.set_rules(dec.suppressed or [], dec.blank_ids or [])
        tokens = np.asarray([dec.initial], np.int64)
        for step in range(WG.TINY["steps"] + 1):
            t.decode(tokens if step == 0 else tokens[:, -1:], first=(step == 0), sot_index=dec.sot_index)
            tok, _lp = t.pick_greedy(**dec._pick_state(tokens))
            tokens = np.concatenate([tokens, [[tok]]], axis=1)
        assert min(t.margins) >= WG.MARGIN, (seconds, seed, [f"{m:.2e}" for m in t.margins])
        worst = min(worst, min(t.margins))
    print(f"worst margin {worst:.3e}")
