"""Window groups on the GPU (csrc/window_group.hip, csrc/select.hip: rules_pick_rows_kernel; whisperlivekit_amd/transcribe.py:
decode_many / WindowStacker): the greedy temperature-0 steps of up to 8 batch-Whisper windows in one launch chain.

  1. the rows pick gives wlk_pick_greedy's token and log-probability bit for bit, and the host rules' within 2e-6;
  2. a row's logits, pick, KV cache and following steps do not depend on the rows stacked beside it (bit-identical to the
     same window stepped in a group of one);
  3. against the solo step (wlk_decode of one token + wlk_pick_greedy) the token ids are identical and the
     log-probabilities within 5e-4 (the solo step folds the cross-attention's query projection and the merge of its key
     splits into neighbouring kernels, the group keeps the multi-row forms; the worst difference seen is printed);
  4. the windows are those of tests/window_group_cases.py, whose decisions the CPU oracle keeps >= 1e-3 clear of a flip
     (tests/test_window_stack_cpu.py), so nothing here allows for ties;
  5. a call the host checks refuse has launched nothing and advanced nobody."""
import copy
import threading

import numpy as np
import pytest
import torch

import helpers as H
import window_group_cases as WG
from whisperlivekit_amd import _lib, synth, transcribe as TR

pytestmark = pytest.mark.gpu
KAT = H.golden_json("transcribe_kat.json")
LOGPROB_ATOL = 5e-4          # test_transcribe.compare_result's allowance for log-probabilities
ERR_ARG, ERR_STATE = -1, -3


@pytest.fixture()
def real_vocab(tmp_path, monkeypatch):
    monkeypatch.setenv("WLK_VOCAB_DIR", H.real_vocab_dir(tmp_path))
    monkeypatch.setenv("WLK_SYNTHETIC_VOCAB", "0")
    monkeypatch.delenv("WLK_TRANSCRIBE_STACK", raising=False)


def _histories(dec, rng):
    """tests/test_gpu_transcribe_rules.py's: sampled-token histories that walk every branch of ApplyTimestampRules."""
    tb, eot = dec.tok.timestamp_begin, dec.tok.eot
    text = lambda n: [int(t) for t in rng.integers(300, 20000, n)]
    return [[], [tb], [tb + 3], [tb, *text(3)], [tb, *text(2), tb + 40], [tb, *text(2), tb + 40, tb + 40],
            [tb, *text(1), tb + 40, tb + 40, *text(2)], [tb, *text(4), tb + 1499], [tb, *text(2), tb + 700, tb + 700, eot],
            text(5), [tb + 1500], [tb, *text(2), tb + 1500, tb + 1500]]


# ---- 1. the rows kernel against the one-row kernel and the host rules -----------------------------------------------------------
@pytest.mark.parametrize("options", [dict(), dict(without_timestamps=True), dict(suppress_blank=False, suppress_tokens=""),
                                     dict(max_initial_timestamp=None), dict(prompt="hello there", suppress_tokens="1,2,-1")])
def test_rows_pick_equals_the_one_row_pick_and_the_host_rules(options, real_vocab):
    from whisperlivekit_amd.engine import HipWhisperModel, pick_rows
    model = HipWhisperModel.synthetic("micro", 3, device=0)
    rng = np.random.default_rng(11)
    try:
        dec = TR._WindowDecoder(model, TR.DecodingOptions(language="en", temperature=0.0, **options))
        V = model.dims.n_vocab
        s = TR._rows_of(model).get(1)
        s.encode_mel(TR.pad_or_trim(s.log_mel(synth.speech_like(7.0, seed=5))))
        base = (dec.suppressed or [], dec.blank_ids or [])
        s.set_rules(*base)
        rows = []                      # (logits, state, rule lists, wlk_pick_greedy's (token, logprob), the host rules' (token, logprob))

        def host(d, logits, tokens):
            x = logits.copy()[None]
            lp = d._apply_rules(x, tokens)
            tok = int(torch.from_numpy(x).argmax(dim=-1)[0])
            assert np.isfinite(lp[0, tok])
            return tok, float(lp[0, tok])
        for hi, hist in enumerate(_histories(dec, rng)):
            tokens = np.asarray([list(dec.initial) + hist], np.int64)
            s.decode(tokens, first=True, sot_index=dec.sot_index)
            state = dec._pick_state(tokens)
            logits = TR._logits(s, 1, V)[0].copy()
            rows.append((logits, state, base, s.pick_greedy(**state), host(dec, logits, tokens)))
            if hi in (3, 9):           # the same row under ANOTHER suppress list: the first list's winner goes
                d2 = copy.copy(dec)
                d2.suppressed = sorted(set(dec.suppressed or []) | {rows[-1][4][0]})
                other = (d2.suppressed, base[1])
                s.set_rules(*other)
                rows.append((logits, state, other, s.pick_greedy(**state), host(d2, logits, tokens)))
                assert rows[-1][3][0] != rows[-2][3][0]
                s.set_rules(*base)
        assert len(rows) == 14
        n_launches = 0
        for order_seed, sizes in ((1, (1, 2, 3, 8)), (2, (5, 8, 1))):
            order = np.random.default_rng(order_seed).permutation(len(rows))
            at = 0
            for n in sizes:
                part = [rows[i] for i in order[at:at + n]]
                at += n
                lists = []
                for r in part:
                    if r[2] not in lists:
                        lists.append(r[2])
                masks = np.stack([WG.rules_mask(V, *l) for l in lists])
                toks, lps = pick_rows(np.stack([r[0] for r in part]), masks, [lists.index(r[2]) for r in part],
                                      [r[1] for r in part])
                n_launches += 1
                for k, r in enumerate(part):
                    assert (int(toks[k]), float(lps[k])) == r[3], (options, n, k, (toks[k], lps[k]), r[3])
                    assert int(toks[k]) == r[4][0]
                    assert float(lps[k]) == pytest.approx(r[4][1], abs=2e-6)
            assert at == len(rows)
        assert n_launches == 7
    finally:
        TR.release_sessions(model)
        model.close()


# ---- 2. / 3. a group of n against a group of one and against the solo step ------------------------------------------------------
class _Runs:
    """The eight windows of window_group_cases stepped (a) each in a group of one, (b) each by the solo step: computed once,
    read by every stacked case."""

    def __init__(self, tmp_dir):
        from whisperlivekit_amd.engine import HipWhisperModel, HipWindowGroup
        self.mp = pytest.MonkeyPatch()
        self.mp.setenv("WLK_VOCAB_DIR", H.real_vocab_dir(tmp_dir))
        self.mp.setenv("WLK_SYNTHETIC_VOCAB", "0")
        self.model = HipWhisperModel.synthetic(WG.MODEL, WG.SEED, device=0)
        self.group = HipWindowGroup(self.model, 8)
        self.sessions = []
        self.mels = {}
        self.alone = self.run(range(len(WG.WINDOWS)), "alone")
        self.solo = self.run(range(len(WG.WINDOWS)), "solo")

    def session(self):
        s = self.model.new_session(beam=1, max_audio_seconds=1.0, batched=False)
        self.sessions.append(s)
        return s

    def run(self, indices, how):
        """-> ([Win], rows per step); how: "stacked" (all live windows in one call), "alone" (one call per window), "solo"
        (wlk_decode + wlk_pick_greedy).  Win.extra holds the logits row of every own step."""
        V = self.model.dims.n_vocab
        wins = [WG.Win(i, WG.WINDOWS[i], self.model, self.session()) for i in indices]

        def open_window(w):
            s = w.session
            if w.index not in self.mels:
                self.mels[w.index] = TR.pad_or_trim(s.log_mel(WG.window_audio(w.spec)))
            s.encode_mel(self.mels[w.index])
            s.set_rules(*w.rules())
            s.decode(w.tokens, first=True, sot_index=w.dec.sot_index)
            return (*s.pick_greedy(**w.dec._pick_state(w.tokens)), TR._logits(s, 1, V)[0].copy())

        def stacked(live):
            toks, lps = self.group.step_pick([w.session for w in live], [int(w.tokens[0, -1]) for w in live],
                                             [w.dec._pick_state(w.tokens) for w in live])
            return [(toks[r], lps[r], self.group.export_logits(r).copy()) for r in range(len(live))]

        def step(live):
            if how == "stacked":
                return stacked(live)
            if how == "alone":
                return [stacked([w])[0] for w in live]
            out = []
            for w in live:
                w.session.decode(w.tokens[:, -1:], first=False)
                out.append((*w.session.pick_greedy(**w.dec._pick_state(w.tokens)), TR._logits(w.session, 1, V)[0].copy()))
            return out
        sizes = WG.drive(wins, open_window, step, lambda w: w.session.set_rules(*w.eot_only_rules(V)))
        for w in wins:
            w.kv = [w.session.export(f"self_{kv}:{layer}") for layer in range(self.model.dims.n_text_layer) for kv in "kv"]
        return wins, sizes

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


def test_the_eight_windows_against_the_solo_step(runs):
    """Contract 3 for every window on its own (a group of one against wlk_decode + wlk_pick_greedy)."""
    worst_lp = worst_logit = 0.0
    for a, b in zip(runs.alone[0], runs.solo[0]):
        assert [t for t, _ in a.picks] == [t for t, _ in b.picks], a.index
        assert len(a.picks) == min(a.spec["sample_len"], 5 if "force_eot" in a.spec else 10 ** 6,
                                   2 if a.spec["prompt"] == "full" else 10 ** 6)
        for (_, la), (_, lb), xa, xb in zip(a.picks, b.picks, a.extra, b.extra):
            worst_lp = max(worst_lp, abs(la - lb))
            worst_logit = max(worst_logit, float(np.abs(xa - xb).max()))
            assert abs(la - lb) <= LOGPROB_ATOL, (a.index, la, lb)
    print(f"\ngroup of one against the solo step: worst log-probability difference {worst_lp:.3e}, worst logit difference "
          f"{worst_logit:.3e} over {sum(len(w.picks) for w in runs.alone[0])} steps of {len(runs.alone[0])} windows")


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
def test_a_row_does_not_depend_on_the_rows_beside_it(n, runs):
    """Contracts 2 and 3: the first n windows in one group (they join at iterations 0-2 and leave at sample_len, at a
    forced <|endoftext|> and at n_ctx) against each of them in a group of one - logits, token, log-probability at every
    step and the KV cache at the end bit for bit - and against the solo step."""
    wins, sizes = runs.run(range(n), "stacked")
    assert max(sizes) == n and (n == 1 or len(set(sizes)) > 1), sizes
    worst = 0.0
    for w, a, b in zip(wins, runs.alone[0], runs.solo[0]):
        assert w.picks == a.picks, (n, w.index)
        assert len(w.extra) == len(a.extra)
        for step, (x, y) in enumerate(zip(w.extra, a.extra)):
            assert np.array_equal(x, y), (n, w.index, step, float(np.abs(x - y).max()))
        for x, y in zip(w.kv, a.kv):
            assert x.size > 0 and np.array_equal(x, y), (n, w.index)
        assert [t for t, _ in w.picks] == [t for t, _ in b.picks]
        worst = max([worst] + [abs(p[1] - q[1]) for p, q in zip(w.picks, b.picks)])
    assert worst <= LOGPROB_ATOL
    print(f"\n{n} windows, rows per step {sizes}: worst log-probability difference to the solo step {worst:.3e}")


def test_one_case_on_tiny_en_dimensions(real_vocab):
    """Six layers, six heads, d = 384 (the GEMV's partly filled last chunk): three windows stacked against each alone and
    against the solo step."""
    from whisperlivekit_amd.engine import HipWhisperModel, HipWindowGroup
    model = HipWhisperModel.synthetic(WG.TINY["model"], WG.TINY["seed"], device=0)
    group = HipWindowGroup(model, 4)
    V = model.dims.n_vocab
    sessions = []
    try:
        eot = TR._tokenizer_for(model, "en", "transcribe").eot
        dec = TR._WindowDecoder(model, TR.DecodingOptions(language="en", temperature=0.0, suppress_tokens=f"-1,{eot}"))
        mels = None

        def run(how):
            nonlocal mels
            ss = [model.new_session(beam=1, max_audio_seconds=1.0, batched=False) for _ in range(3)]
            sessions.extend(ss)
            if mels is None:
                mels = [TR.pad_or_trim(ss[0].log_mel(synth.speech_like(sec, seed=sd))) for sec, sd in WG.TINY["audios"]]
            toks = [np.asarray([dec.initial], np.int64) for _ in ss]
            rec = [[] for _ in ss]
            for i, s in enumerate(ss):
                s.encode_mel(mels[i])
                s.set_rules(dec.suppressed or [], dec.blank_ids or [])
                s.decode(toks[i], first=True, sot_index=dec.sot_index)
                t, lp = s.pick_greedy(**dec._pick_state(toks[i]))
                toks[i] = np.concatenate([toks[i], [[t]]], axis=1)
            for _step in range(WG.TINY["steps"]):
                states = [dec._pick_state(t) for t in toks]
                if how == "stacked":
                    got_t, got_lp = group.step_pick(ss, [int(t[0, -1]) for t in toks], states)
                    res = [(int(got_t[r]), float(got_lp[r]), group.export_logits(r).copy()) for r in range(3)]
                elif how == "alone":
                    res = []
                    for i, s in enumerate(ss):
                        got_t, got_lp = group.step_pick([s], [int(toks[i][0, -1])], [states[i]])
                        res.append((int(got_t[0]), float(got_lp[0]), group.export_logits(0).copy()))
                else:
                    res = []
                    for i, s in enumerate(ss):
                        s.decode(toks[i][:, -1:], first=False)
                        res.append((*s.pick_greedy(**states[i]), TR._logits(s, 1, V)[0].copy()))
                for i, r in enumerate(res):
                    rec[i].append(r)
                    toks[i] = np.concatenate([toks[i], [[r[0]]]], axis=1)
            return rec
        stacked, alone, solo = run("stacked"), run("alone"), run("solo")
        worst = 0.0
        for i in range(3):
            for a, b, c in zip(stacked[i], alone[i], solo[i]):
                assert a[:2] == b[:2] and np.array_equal(a[2], b[2]), i
                assert a[0] == c[0] and abs(a[1] - c[1]) <= LOGPROB_ATOL, (i, a[:2], c[:2])
                worst = max(worst, abs(a[1] - c[1]))
        print(f"\ntiny.en: worst log-probability difference to the solo step {worst:.3e}")
    finally:
        for s in sessions:
            s.close()
        group.close()
        model.close()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------
def _refused(fn, code):
    with pytest.raises(_lib.WlkError) as e:
        fn()
    assert e.value.code == code, (e.value.code, str(e.value))


def test_the_last_position_is_taken_inside_a_group_and_the_next_call_is_refused(runs):
    """A session at self_len == n_text_ctx - 1 takes its last step beside another one; the next call with it is refused
    with WLK_ERR_STATE before anything is launched, and the other session - and its twin, which never met the refused
    call - go on to the same bits, stacked and solo."""
    V, n_ctx = runs.model.dims.n_vocab, runs.model.dims.n_text_ctx
    full = WG.Win(3, WG.WINDOWS[3], runs.model, runs.session())
    pair = [WG.Win(0, WG.WINDOWS[0], runs.model, runs.session()) for _ in range(2)]
    for w in [full] + pair:
        s = w.session
        s.encode_mel(runs.mels[w.index])
        s.set_rules(*w.rules())
        s.decode(w.tokens, first=True, sot_index=w.dec.sot_index)
        w.take(*s.pick_greedy(**w.dec._pick_state(w.tokens)))
    assert full.tokens.shape[1] == n_ctx                 # n_ctx - 1 positions are in the cache, the last token is still to be fed
    good, twin = pair

    def step(ws):
        toks, lps = runs.group.step_pick([w.session for w in ws], [int(w.tokens[0, -1]) for w in ws],
                                         [w.dec._pick_state(w.tokens) for w in ws])
        logits = [runs.group.export_logits(r).copy() for r in range(len(ws))]
        for w, t, lp in zip(ws, toks, lps):
            w.take(t, lp)
        return logits
    a = step([full, good])
    b = step([twin])
    assert np.array_equal(a[1], b[0]) and good.picks == twin.picks
    assert full.picks[1] == runs.alone[0][3].picks[1]
    before = runs.group.stats()
    _refused(lambda: step([full, good]), ERR_STATE)
    _refused(lambda: step([good, full]), ERR_STATE)
    assert runs.group.stats() == before and good.picks == twin.picks
    assert np.array_equal(step([good])[0], step([twin])[0]) and good.picks == twin.picks
    for w in (good, twin):                              # ... and a following solo step of each
        w.session.decode(w.tokens[:, -1:], first=False)
    assert np.array_equal(TR._logits(good.session, 1, V), TR._logits(twin.session, 1, V))


def test_bad_arguments_are_refused_without_a_state_change(runs, real_vocab):
    from whisperlivekit_amd.engine import HipWhisperModel
    model, group = runs.model, runs.group
    V = model.dims.n_vocab
    good, twin = [WG.Win(0, WG.WINDOWS[0], model, runs.session()) for _ in range(2)]
    for w in (good, twin):
        s = w.session
        s.encode_mel(runs.mels[0])
        s.set_rules(*w.rules())
        s.decode(w.tokens, first=True, sot_index=w.dec.sot_index)
        w.take(*s.pick_greedy(**w.dec._pick_state(w.tokens)))
    tok, st = int(good.tokens[0, -1]), good.dec._pick_state(good.tokens)
    beam2 = model.new_session(beam=2, max_audio_seconds=1.0, batched=False)
    unprefilled, unruled = runs.session(), runs.session()
    attached = model.new_session(beam=1, max_audio_seconds=1.0, batched=True)       # its steps belong to the batch engine's loops
    other_model = HipWhisperModel.synthetic(WG.MODEL, WG.SEED + 1, device=0)
    foreign = other_model.new_session(beam=1, max_audio_seconds=1.0, batched=False)
    try:
        beam2.encode_mel(runs.mels[0])
        beam2.set_rules(*good.rules())
        beam2.decode(np.tile(good.tokens[:, :-1], (2, 1)), first=True, sot_index=good.dec.sot_index)
        unprefilled.encode_mel(runs.mels[0])
        unprefilled.set_rules(*good.rules())
        unruled.encode_mel(runs.mels[0])
        unruled.decode(good.tokens[:, :-1], first=True, sot_index=good.dec.sot_index)
        attached.encode_mel(runs.mels[0])
        attached.set_rules(*good.rules())
        attached.decode(good.tokens[:, :-1], first=True, sot_index=good.dec.sot_index)
        foreign.encode_mel(runs.mels[0])
        foreign.set_rules(*good.rules())
        foreign.decode(good.tokens[:, :-1], first=True, sot_index=good.dec.sot_index)
        before = group.stats()
        g = good.session
        _refused(lambda: group.step_pick([g, g], [tok, tok], [st, st]), ERR_ARG)                       # listed twice
        _refused(lambda: group.step_pick([g, beam2], [tok, tok], [st, st]), ERR_ARG)                   # two rows
        _refused(lambda: group.step_pick([g, unprefilled], [tok, tok], [st, st]), ERR_STATE)           # before its prefill
        _refused(lambda: group.step_pick([g, unruled], [tok, tok], [st, st]), ERR_STATE)               # without rules
        _refused(lambda: group.step_pick([g, foreign], [tok, tok], [st, st]), ERR_ARG)                 # another model's
        _refused(lambda: group.step_pick([g, attached], [tok, tok], [st, st]), ERR_STATE)              # attached to the engine
        _refused(lambda: group.step_pick([], [], []), ERR_ARG)                                         # n = 0
        _refused(lambda: group.step_pick([g] * 9, [tok] * 9, [st] * 9), ERR_ARG)                       # n = 9
        _refused(lambda: group.step_pick([g], [V], [st]), ERR_ARG)                                     # token out of range
        _refused(lambda: group.step_pick([g], [tok], [dict(st, ts_mode=3)]), ERR_ARG)                  # rule parameters
        assert group.stats() == before
        for w in (good, twin):                          # `good` goes on as its twin, which met none of the refused calls
            toks, lps = group.step_pick([w.session], [int(w.tokens[0, -1])], [w.dec._pick_state(w.tokens)])
            w.extra.append(group.export_logits(0).copy())
            w.take(toks[0], lps[0])
        assert good.picks == twin.picks and np.array_equal(good.extra[-2], twin.extra[-2])
        assert np.array_equal(good.session.export("self_k:0"), twin.session.export("self_k:0"))
    finally:
        beam2.close()
        attached.close()
        foreign.close()
        other_model.close()


# ---- decode_many, the stacker under threads, the reference's recordings -------------------------------------------------------
def _same_result(got, want):
    assert (got.tokens, got.text, got.no_speech_prob, got.language, got.temperature) == \
        (want.tokens, want.text, want.no_speech_prob, want.language, want.temperature)
    assert got.avg_logprob == pytest.approx(want.avg_logprob, abs=LOGPROB_ATOL)
    assert got.compression_ratio == want.compression_ratio


@pytest.mark.parametrize("opts", WG.DECODE_MANY_OPTIONS, ids=["plain", "no-eot"])
def test_decode_many_equals_decode_per_window(opts, real_vocab):
    """Five windows - a silent one, ones that end at once, different lengths of speech - through decode_many against five
    decode() calls."""
    from whisperlivekit_amd.engine import HipWhisperModel
    model = HipWhisperModel.synthetic(WG.MODEL, WG.SEED, device=0)
    try:
        s = TR._rows_of(model).get(1)
        mels = [np.zeros((80, 3000), np.float32)] + [TR.pad_or_trim(s.log_mel(WG.window_audio(sp))) for sp in WG.DECODE_MANY_WINDOWS]
        options = TR.DecodingOptions(**opts)
        want = [TR.decode(model, m, options) for m in mels]
        got = TR.decode_many(model, mels, options)
        for g, w in zip(got, want):
            _same_result(g, w)
        st = TR.window_stacker(model).stats()        # a window left alone in flight goes on by its session's own steps
        assert st["rows"] + st["solo_steps"] == sum(min(len(w.tokens) + 1, opts["sample_len"]) - 1 for w in want)
        if opts.get("suppress_tokens"):
            assert st["mean_rows_per_step"] == len(mels) and st["solo_steps"] == 0
    finally:
        TR.release_sessions(model)
        model.close()


def test_a_single_window_steps_on_its_own_chain_and_gives_the_group_steps_result(real_vocab):
    """The front's default sends a window that is alone in flight through its session's own step; contract 3 holds across
    that switch: the same tokens, log-probabilities within the solo allowance, against a front that uses the group."""
    from whisperlivekit_amd.engine import HipWhisperModel
    model = HipWhisperModel.synthetic(WG.MODEL, WG.SEED, device=0)
    try:
        s = TR._rows_of(model).get(1)
        mel = TR.pad_or_trim(s.log_mel(WG.window_audio(WG.WINDOWS[0])))
        options = TR.DecodingOptions(**WG.DECODE_MANY_OPTIONS[1])
        want = TR.decode(model, mel, options)
        own = TR.decode_many(model, [mel], options)[0]
        st = TR.window_stacker(model)
        assert own == want and st.stats()["steps"] == 0 and st.solo_steps == options.sample_len - 1
        grouped = TR.decode_many(model, [mel], options, stacker=TR.WindowStacker(model, 8, group=st.group, solo_single=False))[0]
        assert st.group.stats()["rows"] == options.sample_len - 1
        _same_result(grouped, want)
    finally:
        TR.release_sessions(model)
        model.close()


def test_the_stacker_under_threads(real_vocab, monkeypatch):
    """Eight threads transcribe eight recordings on one model with WLK_TRANSCRIBE_STACK=8: the result dictionaries are
    those of the serial, unstacked runs, the group's steps carried more than one row on average, and a window whose
    session has no text position left raises in its own thread only."""
    from test_transcribe import compare_result
    from whisperlivekit_amd.engine import HipWhisperModel
    model = HipWhisperModel.synthetic(WG.MODEL, WG.SEED, device=0)
    try:
        audios = [WG.window_audio(sp) for sp in WG.WINDOWS]
        want = [TR.transcribe(model, a, **WG.TRANSCRIBE_KW) for a in audios]
        assert TR.window_stacker(model) is None
        TR.set_stack(model, TR.resolve_stack(None))            # as HipWhisperASR(stack=None) with the variable unset: off
        assert TR.transcribe(model, audios[0], **WG.TRANSCRIBE_KW) == want[0] and TR.window_stacker(model) is None
        monkeypatch.setenv("WLK_TRANSCRIBE_STACK", "8")
        model.__dict__.pop("_window_stack_rows")
        got = [None] * len(audios)
        errors = [None] * (len(audios) + 1)
        start = threading.Barrier(len(audios) + 1)

        def work(i):
            try:
                start.wait(60)
                got[i] = TR.transcribe(model, audios[i], **WG.TRANSCRIBE_KW)
            except BaseException as e:
                errors[i] = e

        def doomed():
            s = model.new_session(beam=1, max_audio_seconds=1.0, batched=False)
            try:
                w = WG.Win(3, WG.WINDOWS[3], model, s)
                s.encode_mel(TR.pad_or_trim(s.log_mel(audios[3])))
                s.set_rules(*w.rules())
                full = np.concatenate([w.tokens, w.tokens[:, -1:]], axis=1)      # n_text_ctx tokens: no position left
                s.decode(full, first=True, sot_index=w.dec.sot_index)
                start.wait(60)
                TR.window_stacker(model, 8).run(TR._GreedyWindow(w.dec, s, full, np.zeros(1, np.float32), 3))
            except BaseException as e:
                errors[-1] = e
            finally:
                s.close()
        ts = [threading.Thread(target=work, args=(i,)) for i in range(len(audios))] + [threading.Thread(target=doomed)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(120)
        assert not any(t.is_alive() for t in ts)
        assert errors[:-1] == [None] * len(audios), errors
        # refused by the group's host checks (WLK_ERR_STATE) or, if it happened to be alone in flight, by its session's own
        # step (wlk_decode: WLK_ERR_CAPACITY)
        assert isinstance(errors[-1], _lib.WlkError) and errors[-1].code in (ERR_STATE, -4), errors[-1]
        for g, w in zip(got, want):
            compare_result(g, w)
        st = TR.window_stacker(model).stats()
        print(f"\n8 threads: {st}")
        assert st["steps"] > 0 and st["mean_rows_per_step"] > 1.0, st
    finally:
        TR.release_sessions(model)
        model.close()


@pytest.mark.parametrize("case", [c for c in KAT if all(call["temperature"] == 0 and call["beam"] is None for call in c["calls"])],
                         ids=lambda c: c["name"])
def test_the_references_recordings_through_one_stacker(case, real_vocab):
    """The greedy temperature-0 cases of tests/golden/transcribe_kat.json.gz (test_gpu_transcribe_rules.py's selection), each
    transcribed by three threads at once through one stacker: every one is the reference's result."""
    from test_transcribe import compare_result, make_audio
    from whisperlivekit_amd.engine import HipWhisperModel
    model = HipWhisperModel.synthetic(case["model"], 0, device=0)
    try:
        TR.set_stack(model, 4)
        kwargs = dict(case["kwargs"])
        audio = make_audio(case["audio"])
        got, errors = [None] * 3, [None] * 3

        def work(i):
            try:
                got[i] = TR.transcribe(model, audio, **kwargs)
            except BaseException as e:
                errors[i] = e
        ts = [threading.Thread(target=work, args=(i,)) for i in range(3)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(120)
        assert not any(t.is_alive() for t in ts) and errors == [None] * 3, errors
        for g in got:
            compare_result(g, case["result"])
        st = TR.window_stacker(model).stats()
        print(f"\n{case['name']}: {st}")
        assert st["steps"] + st["solo_steps"] > 0 and st["windows"] >= 3, st
    finally:
        TR.release_sessions(model)
        model.close()
