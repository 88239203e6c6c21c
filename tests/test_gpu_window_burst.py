"""Bursts of greedy steps on the GPU (csrc/window_group.hip: wlk_group_run_pick, group_advance_rows_kernel; csrc/common.h:
pick_rules_advance, step_row_scalars; whisperlivekit_amd/transcribe.py: WindowStacker(burst=k)): up to 16 steps of up to 8
windows behind one library call, the next step of every row derived on the device.

  1. the device's rule transition gives `_pick_state(history + [token])` field for field;
  2. a burst gives, bit for bit, what the same window gives stepped alone with one wlk_group_step_pick per token: token,
     log-probability and the number of steps at every call, every self-attention K/V export, the logits row and the
     alignment-window export at the end - for rows that end by budget, by <|endoftext|> in the middle of a burst and by
     context room in the middle of a burst, each beside rows that go on (and repeat their last step as dead rows);
  3. output entries behind a row's last step, and guard words behind the three output arrays, are untouched;
  4. after a burst a session goes on, stacked or solo, to the bits of a twin that never rode one;
  5. a call the host checks refuse has launched nothing and advanced nobody;
  6. the windows are those of tests/window_burst_cases.py, whose decisions the CPU oracle keeps >= 1e-3 clear of a flip
     (tests/test_window_burst_cpu.py), so nothing here allows for ties."""
import ctypes as C
import threading

import numpy as np
import pytest

import helpers as H
import window_burst_cases as WB
import window_group_cases as WG
from whisperlivekit_amd import _lib, synth, transcribe as TR

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -3
SENTINEL_TOKEN, SENTINEL_LP, GUARD = -77, np.float32(123.5), 0x5A5A5A5A
N_GUARD = 8


@pytest.fixture()
def real_vocab(tmp_path, monkeypatch):
    monkeypatch.setenv("WLK_VOCAB_DIR", H.real_vocab_dir(tmp_path))
    monkeypatch.setenv("WLK_SYNTHETIC_VOCAB", "0")
    monkeypatch.delenv("WLK_TRANSCRIBE_STACK", raising=False)
    monkeypatch.delenv("WLK_TRANSCRIBE_STACK_BURST", raising=False)


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def raw_run_pick(group, sessions, tokens, states, max_steps, burst):
    """wlk_group_run_pick over arrays the test owns: sentinels in every output entry, guard words behind all three arrays.
    -> (ids [n][burst], log-probabilities [n][burst], steps [n]) after contract 3 has been checked."""
    from whisperlivekit_amd.engine import HipSession
    n, width = len(sessions), max(int(burst), 1)
    handles = (C.c_void_p * max(n, 1))(*[s._h for s in sessions])
    tok = np.ascontiguousarray(tokens, dtype=np.int64).reshape(-1)
    prm = np.asarray([[int(st[f]) for f in HipSession.PICK_FIELDS] for st in states], dtype=np.int32).reshape(-1, 8)
    lim = np.ascontiguousarray(max_steps, dtype=np.int32).reshape(-1)
    ids = np.full(max(n, 1) * width + N_GUARD, SENTINEL_TOKEN, np.int32)
    lps = np.full(max(n, 1) * width + N_GUARD, SENTINEL_LP, np.float32)
    steps = np.full(max(n, 1) + N_GUARD, GUARD, np.uint32)
    ids[-N_GUARD:] = GUARD
    lps[-N_GUARD:].view(np.uint32)[:] = GUARD
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    _lib.check(group.lib.wlk_group_run_pick(group._h, handles, vp(tok), vp(prm), vp(lim), n, int(burst), vp(ids), vp(lps), vp(steps)))
    assert (ids[-N_GUARD:] == GUARD).all() and (lps[-N_GUARD:].view(np.uint32) == GUARD).all() and (steps[n:] == GUARD).all()
    took = steps[:n].astype(np.int64)
    ids, lps = ids[:n * width].reshape(n, width), lps[:n * width].reshape(n, width)
    for r in range(n):
        assert 1 <= took[r] <= min(width, lim[r]), (r, took[r])
        assert (ids[r, took[r]:] == SENTINEL_TOKEN).all() and (bits(lps[r, took[r]:]) == bits(SENTINEL_LP)).all(), r
        assert (ids[r, :took[r]] >= 0).all()
    return ids, lps, took


class _Runs:
    """micro.en, one group of 8 rows, and the eight windows of window_burst_cases each stepped alone with one step_pick per
    token: computed once, read by every burst case."""

    def __init__(self, tmp_dir):
        from whisperlivekit_amd.engine import HipWhisperModel, HipWindowGroup
        self.mp = pytest.MonkeyPatch()
        self.mp.setenv("WLK_VOCAB_DIR", H.real_vocab_dir(tmp_dir))
        self.mp.setenv("WLK_SYNTHETIC_VOCAB", "0")
        self.model = HipWhisperModel.synthetic(WB.MODEL, WB.SEED, device=0)
        self.group = HipWindowGroup(self.model, 8)
        self.sessions, self.mels = [], {}
        self.alone = [self.step_alone(self.open(i)) for i in range(len(WB.WINDOWS))]

    def session(self):
        s = self.model.new_session(beam=1, max_audio_seconds=1.0, batched=False)
        self.sessions.append(s)
        return s

    def open(self, index):
        """-> the window behind its prefill and the prefill's own pick"""
        w = WB.Win(index, WB.WINDOWS[index], self.model, self.session())
        s = w.session
        if index not in self.mels:
            self.mels[index] = TR.pad_or_trim(s.log_mel(WG.window_audio(w.spec)))
        s.encode_mel(self.mels[index])
        s.set_rules(*w.rules())
        s.decode(w.tokens, first=True, sot_index=w.dec.sot_index)
        w.take(*s.pick_greedy(**w.dec._pick_state(w.tokens)))
        return w

    def single(self, w):
        """one step_pick of `w` in a group of one"""
        toks, lps = self.group.step_pick([w.session], [int(w.tokens[0, -1])], [w.dec._pick_state(w.tokens)])
        w.take(toks[0], lps[0], self.group.export_logits(0).copy())

    def step_alone(self, w, n=10 ** 6):
        while not w.over and n > 0:
            self.single(w)
            n -= 1
        self.exports(w)
        return w

    def exports(self, w):
        s, d = w.session, self.model.dims
        w.kv = [s.export(f"self_{kv}:{layer}") for layer in range(d.n_text_layer) for kv in "kv"]
        w.ring = [s.export(f"xattn_w:{i}") for i in range(len(self.model.alignment_heads))]

    def close(self):
        for s in self.sessions:
            s.close()
        self.group.close()
        self.model.close()
        self.mp.undo()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    r = _Runs(tmp_path_factory.mktemp("vocab"))
    yield r
    r.close()


# ---- 1. the rule transition on the device -------------------------------------------------------------------------------------
def test_the_device_rule_transition_is_the_state_of_the_longer_history(runs):
    from whisperlivekit_amd.engine import HipSession, pick_advance
    cases = WB.transition_cases(runs.model)
    before = [WB.state_of(dec, h) for dec, h, _t in cases]
    got = pick_advance(before, [t for _d, _h, t in cases])
    assert len(got) == len(cases) > 2000
    for (dec, h, t), b, g in zip(cases, before, got):
        want = {f: int(v) for f, v in WB.state_of(dec, h + [t]).items()}
        assert g == want, (h, t, b, g, want)
        assert g == {f: int(v) for f, v in TR._next_pick_state(b, t).items()}
    assert set(got[0]) == set(HipSession.PICK_FIELDS)


# ---- 2. / 3. bursts against single steps --------------------------------------------------------------------------------------
def _burst_drive(runs, indices, burst):
    """The windows `indices` opened, then run_pick calls of `burst` until every window is over; every call is compared
    against the windows stepped alone.  -> [(rows, steps per row)] per call."""
    wins = [runs.open(i) for i in indices]
    for w in wins:
        assert w.picks == runs.alone[w.index].picks[:1]
    calls, first = [], True
    live = [w for w in wins if not w.over]
    while live:
        budgets = [min(WB.FIRST_BUDGET.get(w.index, w.budget()), w.budget()) if first else w.budget() for w in live]
        first = False
        before = runs.group.stats()
        ids, lps, took = raw_run_pick(runs.group, [w.session for w in live], [int(w.tokens[0, -1]) for w in live],
                                      [w.dec._pick_state(w.tokens) for w in live], budgets, burst)
        after = runs.group.stats()
        assert after["steps"] == before["steps"] + burst and after["rows"] == before["rows"] + int(took.sum())
        for r, w in enumerate(live):
            ref, at = runs.alone[w.index], len(w.picks)
            want = ref.picks[at:at + min(budgets[r], burst)]               # the reference ends at <|endoftext|> and at n_ctx
            assert took[r] == len(want), (burst, w.index, at, took[r], len(want))
            assert ids[r, :took[r]].tolist() == [t for t, _ in want], (burst, w.index, at)
            assert bits(lps[r, :took[r]]).tolist() == bits([lp for _, lp in want]).tolist(), (burst, w.index, at)
            # the logits row is that of the row's last OWN step, however many chains it sat through as a dead row
            assert np.array_equal(runs.group.export_logits(r), ref.extra[at + took[r] - 1]), (burst, w.index, at)
            for k in range(took[r]):
                w.take(ids[r, k], lps[r, k])
        calls.append((len(live), took.tolist()))
        live = [w for w in live if not w.over]
        assert len(calls) < 100
    for w in wins:
        ref = runs.alone[w.index]
        assert w.picks == ref.picks and w.tokens.tolist() == ref.tokens.tolist()
        runs.exports(w)
        for x, y in zip(w.kv, ref.kv):
            assert x.size > 0 and np.array_equal(x, y), (burst, w.index)
        assert len(w.ring) == len(ref.ring) > 0
        for x, y in zip(w.ring, ref.ring):
            assert x.size > 0 and np.array_equal(x, y), (burst, w.index)
    return calls


def test_the_reference_ends_every_way_the_burst_cases_need(runs):
    eot = runs.alone[0].dec.tok.eot
    e, f = runs.alone[WB.EOT_WINDOW], runs.alone[WB.FULL_WINDOW]
    assert e.picks[-1][0] == eot and len(e.picks) == 1 + WB.EOT_STEPS
    assert len(f.picks) == 2 and f.tokens.shape[1] == runs.model.dims.n_text_ctx + 1
    assert all(len(w.picks) == w.spec["sample_len"] for w in runs.alone if w is not e and w is not f)


@pytest.mark.parametrize("burst", WB.BURSTS)
@pytest.mark.parametrize("n", sorted(WB.STACKS))
def test_a_burst_gives_the_bits_of_single_steps(n, burst, runs):
    calls = _burst_drive(runs, WB.STACKS[n], burst)
    rows, took = calls[0]
    assert rows == n
    if n == 8:
        # budgets of 1 and 2 beside whole bursts, the context room of ONE position, in one call
        assert took[1] == 1 and took[2] == min(2, burst) and took[WB.FULL_WINDOW] == 1
        assert took[0] == min(burst, WB.WINDOWS[0]["sample_len"] - 1)
        if burst in (5, 16):               # <|endoftext|> in the middle of a burst, beside rows that go on
            at = 0
            for rows, took in calls:
                k = took[-1]               # the <|endoftext|> window is the last row while it lives
                if at + k == WB.EOT_STEPS:
                    assert k < burst and max(took[:-1]) > k, (calls,)
                    break
                at += k
            else:
                raise AssertionError(calls)
    if n == 3 and burst > 1:
        assert took[0] == 1 and took[1] == 1 and took[2] == burst      # context room, budget, a row that goes on


def test_run_pick_of_the_python_front_returns_each_rows_own_steps(runs):
    wins = [runs.open(i) for i in (0, 1, WB.FULL_WINDOW)]
    res = runs.group.run_pick([w.session for w in wins], [int(w.tokens[0, -1]) for w in wins],
                              [w.dec._pick_state(w.tokens) for w in wins], [7, 2, 5], 5)
    assert [len(ids) for ids, _ in res] == [5, 2, 1] and all(ids.dtype == np.int32 and lps.dtype == np.float32 for ids, lps in res)
    for w, (ids, lps) in zip(wins, res):
        want = runs.alone[w.index].picks[1:1 + len(ids)]
        assert ids.tolist() == [t for t, _ in want] and bits(lps).tolist() == bits([lp for _, lp in want]).tolist()
    with pytest.raises(ValueError):
        runs.group.run_pick([wins[0].session], [1, 2], [wins[0].dec._pick_state(wins[0].tokens)], [1], 2)


# ---- 4. after a burst ---------------------------------------------------------------------------------------------------------
def test_after_a_burst_the_sessions_go_on_to_a_twins_bits(runs):
    V = runs.model.dims.n_vocab
    riders, twins = [runs.open(i) for i in (0, 5)], [runs.open(i) for i in (0, 5)]
    ids, lps, took = raw_run_pick(runs.group, [w.session for w in riders], [int(w.tokens[0, -1]) for w in riders],
                                  [w.dec._pick_state(w.tokens) for w in riders], [5, 3], 5)
    assert took.tolist() == [5, 3]
    for r, w in enumerate(riders):
        for k in range(took[r]):
            w.take(ids[r, k], lps[r, k])
    for w, n in zip(twins, took):
        for _ in range(n):
            runs.single(w)
    for w, t in zip(riders, twins):
        assert w.picks == t.picks
        for who in (w, t):                 # a group step, the session's own step, a group step
            runs.single(who)
            who.session.decode(who.tokens[:, -1:], first=False)
            who.take(*who.session.pick_greedy(**who.dec._pick_state(who.tokens)), TR._logits(who.session, 1, V)[0].copy())
            runs.single(who)
        assert len(w.picks) == len(t.picks) == 1 + int(took[riders.index(w)]) + 3
        assert [p[0] for p in w.picks] == [p[0] for p in t.picks]
        assert bits([p[1] for p in w.picks]).tolist() == bits([p[1] for p in t.picks]).tolist()
        for x, y in zip(w.extra[-3:], t.extra[-3:]):
            assert np.array_equal(x, y)
        assert np.array_equal(w.session.export("self_k:0"), t.session.export("self_k:0"))


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------
def _refused(fn, code):
    with pytest.raises(_lib.WlkError) as e:
        fn()
    assert e.value.code == code, (e.value.code, str(e.value))


def test_refused_calls_launch_nothing_and_advance_nobody(runs, real_vocab):
    from whisperlivekit_amd.engine import HipWhisperModel
    model, group = runs.model, runs.group
    V = model.dims.n_vocab
    good, twin = runs.open(0), runs.open(0)
    full = runs.open(WB.FULL_WINDOW)
    runs.single(full)                                    # its last position is taken: no room for another step
    assert full.session and full.tokens.shape[1] == model.dims.n_text_ctx + 1
    tok, st = int(good.tokens[0, -1]), good.dec._pick_state(good.tokens)
    beam2 = model.new_session(beam=2, max_audio_seconds=1.0, batched=False)
    unprefilled, unruled = runs.session(), runs.session()
    attached = model.new_session(beam=1, max_audio_seconds=1.0, batched=True)
    other_model = HipWhisperModel.synthetic(WB.MODEL, WB.SEED + 1, device=0)
    foreign = other_model.new_session(beam=1, max_audio_seconds=1.0, batched=False)
    try:
        prefix = good.tokens[:, :-1]
        beam2.encode_mel(runs.mels[0])
        beam2.set_rules(*good.rules())
        beam2.decode(np.tile(prefix, (2, 1)), first=True, sot_index=good.dec.sot_index)
        unprefilled.encode_mel(runs.mels[0])
        unprefilled.set_rules(*good.rules())
        unruled.encode_mel(runs.mels[0])
        unruled.decode(prefix, first=True, sot_index=good.dec.sot_index)
        for s in (attached, foreign):
            s.encode_mel(runs.mels[0])
            s.set_rules(*good.rules())
            s.decode(prefix, first=True, sot_index=good.dec.sot_index)
        before = group.stats()
        g = good.session
        run = lambda ss, toks, sts, lims, burst: (lambda: group.run_pick(ss, toks, sts, lims, burst))
        _refused(run([g, g], [tok, tok], [st, st], [4, 4], 4), ERR_ARG)                        # listed twice
        _refused(run([g, beam2], [tok, tok], [st, st], [4, 4], 4), ERR_ARG)                    # two rows
        _refused(run([g, unprefilled], [tok, tok], [st, st], [4, 4], 4), ERR_STATE)            # before its prefill
        _refused(run([g, unruled], [tok, tok], [st, st], [4, 4], 4), ERR_STATE)                # without rules
        _refused(run([g, foreign], [tok, tok], [st, st], [4, 4], 4), ERR_ARG)                  # another model's
        _refused(run([g, attached], [tok, tok], [st, st], [4, 4], 4), ERR_STATE)               # attached to the engine
        _refused(run([g, full.session], [tok, tok], [st, st], [4, 4], 4), ERR_STATE)           # text context exceeded
        _refused(run([full.session, g], [tok, tok], [st, st], [4, 4], 4), ERR_STATE)
        _refused(run([], [], [], [], 4), ERR_ARG)                                              # n = 0
        _refused(run([g] * 9, [tok] * 9, [st] * 9, [4] * 9, 4), ERR_ARG)                       # n = 9
        _refused(run([g], [V], [st], [4], 4), ERR_ARG)                                         # token out of range
        _refused(run([g], [tok], [dict(st, ts_mode=3)], [4], 4), ERR_ARG)                      # rule parameters
        _refused(run([g], [tok], [st], [4], 0), ERR_ARG)                                       # burst 0
        _refused(run([g], [tok], [st], [4], 17), ERR_ARG)                                      # burst 17
        _refused(run([g], [tok], [st], [0], 4), ERR_ARG)                                       # a budget of 0
        _refused(run([g, twin.session], [tok, tok], [st, st], [4, -1], 4), ERR_ARG)
        assert group.stats() == before
        # `good` goes on - in a burst - to the bits of its twin, which met none of the refused calls and steps alone
        (ids, lps), = group.run_pick([g], [tok], [st], [3], 16)
        assert len(ids) == 3
        for t, lp in zip(ids, lps):
            good.take(t, lp)
        for _ in range(3):
            runs.single(twin)
        assert good.picks == twin.picks == runs.alone[0].picks[:4]
        assert np.array_equal(group.export_logits(0), twin.extra[-1])
        assert np.array_equal(good.session.export("self_k:0"), twin.session.export("self_k:0"))
    finally:
        beam2.close()
        attached.close()
        foreign.close()
        other_model.close()


# ---- 6. / 7. decode_many and transcribe ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", WG.DECODE_MANY_OPTIONS, ids=["plain", "no-eot"])
def test_decode_many_with_bursts_equals_decode_many_without(opts, real_vocab):
    from whisperlivekit_amd.engine import HipWhisperModel
    model = HipWhisperModel.synthetic(WG.MODEL, WG.SEED, device=0)
    stackers = []
    try:
        s = TR._rows_of(model).get(1)
        mels = [np.zeros((80, 3000), np.float32)] + [TR.pad_or_trim(s.log_mel(WG.window_audio(sp))) for sp in WG.DECODE_MANY_WINDOWS]
        options = TR.DecodingOptions(**opts)
        # solo_single off on both sides: every step of every window is the group's, with or without bursts
        stackers = [TR.WindowStacker(model, 8, solo_single=False, burst=k) for k in (1, 4, 16)]
        want = TR.decode_many(model, mels, options, stacker=stackers[0])
        for st in stackers[1:]:
            got = TR.decode_many(model, mels, options, stacker=st)
            for g, w in zip(got, want):
                assert (g.tokens, g.avg_logprob, g.no_speech_prob, g.text) == (w.tokens, w.avg_logprob, w.no_speech_prob, w.text)
                assert g == w
            a, b = st.group.stats(), stackers[0].group.stats()
            assert a["rows"] == b["rows"] and a["steps"] >= -(-b["steps"] // st.burst)
            if opts.get("suppress_tokens"):            # no window ends early: a call per `burst` steps, no dead rows
                assert a["steps"] == b["steps"] and a["mean_rows_per_step"] == len(mels)
    finally:
        for st in stackers:
            st.close()
        TR.release_sessions(model)
        model.close()


def test_four_threads_transcribe_through_bursts(real_vocab):
    """Four threads of transcribe() on one model with stack 8 and burst 8 against the same four threads with burst 1: the
    same tokens per recording.  Which windows share a call depends on the threads' timing, and a window alone in flight
    takes its session's own step, whose log-probabilities differ from the group's within the solo allowance (contract 3 of
    tests/test_gpu_window_group.py) - so the sums are compared as that file compares them."""
    from test_transcribe import compare_result
    from whisperlivekit_amd.engine import HipWhisperModel
    model = HipWhisperModel.synthetic(WG.MODEL, WG.SEED, device=0)
    try:
        audios = [WG.window_audio(sp) for sp in WG.WINDOWS[:4]]
        TR.set_stack(model, 8)

        def threaded():
            got, errors = [None] * len(audios), [None] * len(audios)
            start = threading.Barrier(len(audios))

            def work(i):
                try:
                    start.wait(60)
                    got[i] = TR.transcribe(model, audios[i], **WG.TRANSCRIBE_KW)
                except BaseException as e:
                    errors[i] = e
            ts = [threading.Thread(target=work, args=(i,)) for i in range(len(audios))]
            for t in ts:
                t.start()
            for t in ts:
                t.join(120)
            assert not any(t.is_alive() for t in ts) and errors == [None] * len(audios), errors
            return got
        assert TR.set_burst(model, 1) == 1
        want = threaded()
        one = TR.window_stacker(model).stats()
        assert TR.set_burst(model, 8) == 8
        got = threaded()
        assert TR.window_stacker(model).burst == 8
        for g, w in zip(got, want):
            assert [seg["tokens"] for seg in g["segments"]] == [seg["tokens"] for seg in w["segments"]] and g["text"] == w["text"]
            compare_result(g, w)
        st = TR.window_stacker(model).stats()
        print(f"\n4 threads: burst 1 {one}, then burst 8 {st}")
        assert st["windows"] == 2 * len(audios)
    finally:
        TR.release_sessions(model)
        model.close()


# ---- 8. tiny.en ---------------------------------------------------------------------------------------------------------------
def test_one_burst_on_tiny_en_dimensions(real_vocab):
    """Six layers, six heads, d = 384: three windows, one burst of six against six single steps, bits."""
    from whisperlivekit_amd.engine import HipWhisperModel, HipWindowGroup
    model = HipWhisperModel.synthetic(WG.TINY["model"], WG.TINY["seed"], device=0)
    group = HipWindowGroup(model, 4)
    sessions = []
    try:
        eot = TR._tokenizer_for(model, "en", "transcribe").eot
        dec = TR._WindowDecoder(model, TR.DecodingOptions(language="en", temperature=0.0, suppress_tokens=f"-1,{eot}"))
        mels, steps = None, WG.TINY["steps"]

        def opened():
            nonlocal mels
            ss = [model.new_session(beam=1, max_audio_seconds=1.0, batched=False) for _ in range(3)]
            sessions.extend(ss)
            if mels is None:
                mels = [TR.pad_or_trim(ss[0].log_mel(synth.speech_like(sec, seed=sd))) for sec, sd in WG.TINY["audios"]]
            toks = []
            for s, mel in zip(ss, mels):
                t = np.asarray([dec.initial], np.int64)
                s.encode_mel(mel)
                s.set_rules(dec.suppressed or [], dec.blank_ids or [])
                s.decode(t, first=True, sot_index=dec.sot_index)
                toks.append(np.concatenate([t, [[s.pick_greedy(**dec._pick_state(t))[0]]]], axis=1))
            return ss, toks
        ss, toks = opened()
        single = [[] for _ in ss]
        for _ in range(steps):
            for i, s in enumerate(ss):
                t, lp = group.step_pick([s], [int(toks[i][0, -1])], [dec._pick_state(toks[i])])
                single[i].append((int(t[0]), float(lp[0])))
                toks[i] = np.concatenate([toks[i], [[int(t[0])]]], axis=1)
        bs, btoks = opened()
        ids, lps, took = raw_run_pick(group, bs, [int(t[0, -1]) for t in btoks], [dec._pick_state(t) for t in btoks], [steps] * 3, steps)
        assert took.tolist() == [steps] * 3
        for i in range(3):
            assert ids[i].tolist() == [t for t, _ in single[i]], i
            assert bits(lps[i]).tolist() == bits([lp for _, lp in single[i]]).tolist(), i
            for layer in range(model.dims.n_text_layer):
                for kv in "kv":
                    assert np.array_equal(bs[i].export(f"self_{kv}:{layer}"), ss[i].export(f"self_{kv}:{layer}")), (i, layer, kv)
    finally:
        for s in sessions:
            s.close()
        group.close()
        model.close()
