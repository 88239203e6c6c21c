"""The host half of draft verification (whisperlivekit_amd/transcribe.py: _accept_draft, clamp_draft, WindowDraft, the draft
of DecodingOptions / decode_many / transcribe; local_agreement.py: HipWhisperASR(draft=...), session_view) over oracle-backed
stand-ins (tests/draft_verify_cases.py), and the decision margins of the windows the GPU tests verify
(tests/test_gpu_draft_verify.py)."""
import numpy as np
import pytest

import draft_verify_cases as DV
import helpers as H
import window_burst_cases as WB
import window_group_cases as WG
from whisperlivekit_amd import local_agreement as LA, synth, transcribe as TR


@pytest.fixture()
def real_vocab(tmp_path, monkeypatch):
    monkeypatch.setenv("WLK_VOCAB_DIR", H.real_vocab_dir(tmp_path))
    monkeypatch.setenv("WLK_SYNTHETIC_VOCAB", "0")
    for name in ("WLK_TRANSCRIBE_STACK", "WLK_TRANSCRIBE_STACK_BURST", "WLK_TRANSCRIBE_DRAFT"):
        monkeypatch.delenv(name, raising=False)


@pytest.fixture()
def model():
    return WG.PickingOracleModel(WG.MODEL, WG.SEED)


def _stacker(model, **kw):
    group = DV.OracleVerifyGroup(8, **kw)
    return TR.WindowStacker(model, 8, group=group, solo_single=False), group


# ---- 1. the acceptance arithmetic ---------------------------------------------------------------------------------------------
EOT = 50256


def _table(tokens, lps):
    return list(zip(tokens, lps))


def test_accept_draft_over_hand_made_pick_tables():
    lps = [-0.25, -1.5, -0.125, -3.0, -0.75]
    draft = [10, 11, 12, 13]
    match = _table([10, 11, 12, 13, 99], lps)
    # no mismatch: everything accepted, next = the pick behind the draft, all five log-probabilities summed
    assert TR._accept_draft(match, draft, EOT) == (4, 99, np.float32(-0.75), np.float32(-5.625))
    # at 0, in the middle, at the last draft position
    assert TR._accept_draft(_table([7, 11, 12, 13, 99], lps), draft, EOT) == (0, 7, np.float32(-0.25), np.float32(-0.25))
    assert TR._accept_draft(_table([10, 11, 8, 13, 99], lps), draft, EOT) == (2, 8, np.float32(-0.125), np.float32(-1.875))
    assert TR._accept_draft(_table([10, 11, 12, 9, 99], lps), draft, EOT) == (3, 9, np.float32(-3.0), np.float32(-4.875))
    # positions behind the first mismatch do not matter
    assert TR._accept_draft(_table([10, 5, 12, 13, 99], lps), draft, EOT)[:2] == (1, 5)
    # <|endoftext|> as the pick inside the draft span: a draft never holds it, so it is the mismatch and the next token
    assert TR._accept_draft(_table([10, EOT, 12, 13, 99], lps), draft, EOT) == (1, EOT, np.float32(-1.5), np.float32(-1.75))
    # the window had ended in front of position 0 (_greedy_take's rule): <|endoftext|> whatever was picked, nothing added
    assert TR._accept_draft(match, draft, EOT, ended=True) == (0, EOT, np.float32(-0.25), np.float32(0.0))
    with pytest.raises(ValueError):
        TR._accept_draft(match, draft[:3], EOT)


def test_the_sum_is_the_greedy_loops_float32_accumulation():
    rng, order_matters = np.random.default_rng(4), False
    for n in (1, 7, 40, 255):
        lps = (-rng.random(n + 1) * 9.0).astype(np.float32)
        draft = [int(t) for t in rng.integers(300, 20000, n)]
        for k in sorted({0, n // 2, n - 1, n}):
            tokens = list(draft) + [777]
            if k < n:
                tokens[k] = DV.wrong(draft[k])
            got = TR._accept_draft(_table(tokens, lps), draft, EOT)
            # the loop of _WindowDecoder.run: one _greedy_take per pick
            toks, total = np.asarray([[1]], np.int64), np.zeros(1, np.float32)
            for j in range(k + 1):
                toks, _over = TR._greedy_take(toks, total, tokens[j], float(lps[j]), EOT, 10 ** 6)
            assert got[0] == k and got[1] == tokens[k]
            assert np.float32(got[3]).view(np.uint32) == total.view(np.uint32)[0], (n, k)
            back = np.float32(0.0)
            for j in range(k, -1, -1):
                back = np.float32(back + lps[j])
            order_matters = order_matters or back != got[3]
    assert order_matters                                      # the cases tell the ascending order from another one


# ---- 2. clamping --------------------------------------------------------------------------------------------------------------
def test_draft_clamping_at_sample_len_n_ctx_and_the_256_row_bound():
    draft = list(range(1000, 1400))
    assert TR.clamp_draft(draft, 3, 224, 448, EOT) == draft[:223]                 # sample_len - 1
    assert TR.clamp_draft(draft, 200, 224, 448, EOT) == draft[:56]                # 256 - P0
    assert TR.clamp_draft(draft, 250, 224, 448, EOT) == draft[:6]
    assert TR.clamp_draft(draft, 256, 224, 448, EOT) == [] and TR.clamp_draft(draft, 300, 224, 448, EOT) == []
    assert TR.clamp_draft(draft, 100, 400, 128, EOT) == draft[:27]                # n_ctx - P0 - 1
    assert TR.clamp_draft(draft, 3, 1, 448, EOT) == []                            # the one sampled token is the first pick
    assert TR.clamp_draft([5, 6, EOT, 7], 3, 224, 448, EOT) == [5, 6]             # a history ends in front of <|endoftext|>
    assert TR.clamp_draft(None, 3, 224, 448, EOT) == [] and TR.clamp_draft([], 3, 224, 448, EOT) == []


# ---- 3. the memory ------------------------------------------------------------------------------------------------------------
def test_window_draft_keeps_a_draft_for_an_extension_and_drops_it_otherwise():
    audio = synth.speech_like(3.0, seed=1)
    mem = TR.WindowDraft()
    assert mem.begin(audio[:16000]) == []                     # nothing remembered yet
    mem.remember([5, 6, 7])
    assert mem.begin(audio[:24000]) == [5, 6, 7] and mem.tokens == []             # an extension; handed out once
    assert np.array_equal(mem.audio, audio[:24000]) and mem.offered == 1
    mem.remember([8, 9])
    assert mem.begin(audio[8000:32000]) == [] and mem.dropped == 1                # trimmed in front
    mem.remember([8, 9])
    other = audio[8000:32000].copy()
    other[100] += 1e-3
    assert mem.begin(other) == [] and mem.dropped == 2                            # one sample differs
    mem.remember([1])
    assert mem.begin(other[:9000]) == [1]                                         # the common prefix is what counts
    mem.remember([1])
    mem.reset()
    assert mem.begin(other) == [] and mem.dropped == 2
    caller = other.copy()
    mem.begin(caller)
    caller[:] = 0.0                                                               # the memory owns its copy
    assert np.array_equal(mem.audio, other)


# ---- 4. decode / decode_many / transcribe over stand-ins ----------------------------------------------------------------------
OPTS = dict(language="en", temperature=0.0, sample_len=12, suppress_tokens=f"-1,{EOT}", without_timestamps=True)


def _mel(model, seconds, seed):
    s = model.new_session()
    return TR.pad_or_trim(s.log_mel(synth.speech_like(seconds, seed=seed)))


def _same(got, want):
    assert got.tokens == want.tokens and got.text == want.text and got.no_speech_prob == want.no_speech_prob
    assert np.float32(got.avg_logprob) == np.float32(want.avg_logprob) and got.compression_ratio == want.compression_ratio


def test_decode_with_a_draft_is_decode_without_one(real_vocab, model):
    mel = _mel(model, 7.0, 5)
    want = TR.decode(model, mel, TR.DecodingOptions(**OPTS))
    assert len(want.tokens) == 12
    truth = want.tokens
    cases = {"right": (truth, 11), "longer than the window": (truth + [500, 501, 502], 11), "wrong at 0": (DV.spoiled(truth, 0), 0),
             "wrong in the middle": (DV.spoiled(truth, 5), 5), "wrong at the last": (DV.spoiled(truth[:11], 10), 10),
             "ends early": (truth[:8] + [EOT, 3], 8)}
    for name, (draft, k) in cases.items():
        stacker, group = _stacker(model)
        got = TR.decode(model, mel, TR.DecodingOptions(**OPTS, draft=draft), stacker=stacker)
        _same(got, want)
        n_d = min(len(TR.clamp_draft(draft, 2, 12, 448, EOT)), 11)
        assert group.verifies == [[(2, n_d, k)]], (name, group.verifies)
        # the steps behind the pass: the window's 12 tokens minus the k + 1 the pass gave
        assert sum(group.calls) == 12 - (k + 1), (name, group.calls)
    # no usable draft, a range the group refuses, no stacker, sampling: today's path, no verify call
    for draft, kw in (([], {}), (None, {}), ([EOT], {}), (truth, dict(low=100))):
        stacker, group = _stacker(model, **kw)
        _same(TR.decode(model, mel, TR.DecodingOptions(**OPTS, draft=draft), stacker=stacker), want)
        assert group.verifies == [] and sum(group.calls) == 11
    _same(TR.decode(model, mel, TR.DecodingOptions(**OPTS, draft=truth)), want)                 # stacking is off
    stacker, group = _stacker(model)
    TR.decode(model, mel, TR.DecodingOptions(**dict(OPTS, temperature=0.4), draft=truth), stacker=stacker)
    TR.decode(model, mel, TR.DecodingOptions(**OPTS, beam_size=2, draft=truth), stacker=stacker)
    assert group.verifies == [] and group.n_calls == 0
    TR.release_sessions(model)


def test_a_verify_call_refused_on_the_host_falls_back_to_the_prefill(real_vocab, model):
    mel = _mel(model, 7.0, 5)
    want = TR.decode(model, mel, TR.DecodingOptions(**OPTS))
    stacker, group = _stacker(model)
    group.verify_fits = lambda a, b: True                     # the pure shape test says yes, the call itself refuses
    group.low = 100
    _same(TR.decode(model, mel, TR.DecodingOptions(**OPTS, draft=want.tokens), stacker=stacker), want)
    assert group.verifies == [] and sum(group.calls) == 11
    TR.release_sessions(model)


def test_decode_many_with_mixed_drafts_is_decode_per_window(real_vocab, model):
    mels = [_mel(model, 4.0, 9), _mel(model, 7.0, 5), _mel(model, 3.0, 6), _mel(model, 6.0, 10)]
    opts = TR.DecodingOptions(**OPTS)
    want = [TR.decode(model, m, opts) for m in mels]
    drafts = [want[0].tokens, None, DV.spoiled(want[2].tokens, 3), []]
    stacker, group = _stacker(model)
    got = TR.decode_many(model, mels, opts, stacker=stacker, drafts=drafts)
    for g, w in zip(got, want):
        _same(g, w)
    assert group.verifies == [[(2, 11, 11), (2, 11, 3)]]      # ONE call for the two windows with a usable draft
    with pytest.raises(ValueError):
        TR.decode_many(model, mels, opts, stacker=stacker, drafts=drafts[:2])
    stacker, group = _stacker(model)
    for g, w in zip(TR.decode_many(model, mels, opts, stacker=stacker, drafts=[None] * 4), want):
        _same(g, w)
    assert group.verifies == []
    TR.release_sessions(model)


KW = dict(language="en", temperature=0.0, sample_len=12, suppress_tokens=f"-1,{EOT}", without_timestamps=True,
          logprob_threshold=None, compression_ratio_threshold=None, no_speech_threshold=None)


def _with_stack(model, monkeypatch):
    group = DV.OracleVerifyGroup(8)
    real = TR.WindowStacker
    monkeypatch.setattr(TR, "WindowStacker", lambda m, rows: real(m, rows, group=group, solo_single=False))
    TR.set_stack(model, 8)
    return group


def test_transcribe_gives_the_same_dictionary_with_and_without_a_draft(real_vocab, model, monkeypatch):
    group = _with_stack(model, monkeypatch)
    audio = synth.speech_like(6.0, seed=5)
    want = TR.transcribe(model, audio, **KW)
    truth = want["segments"][0]["tokens"]
    assert len(truth) == 12 and group.verifies == []
    for draft, k in ((truth, 11), (DV.spoiled(truth, 4), 4), ([], None)):
        mem = TR.WindowDraft()
        mem.begin(audio[:40000])
        mem.remember(draft)
        n = len(group.verifies)
        assert TR.transcribe(model, audio, draft=mem, **KW) == want
        assert group.verifies[n:] == ([[(2, 11, k)]] if k is not None else [])
        assert mem.tokens == truth and np.array_equal(mem.audio, audio)           # this call's first window, for the next
    # a growing buffer through one memory, then a trim
    mem, n = TR.WindowDraft(), len(group.verifies)
    for end in (64000, 72000, 80000):
        assert TR.transcribe(model, audio[:end], draft=mem, **KW) == TR.transcribe(model, audio[:end], **KW)
    assert len(group.verifies) == n + 2 and mem.offered == 2                      # the first call had nothing to verify
    assert TR.transcribe(model, audio[16000:88000], draft=mem, **KW) == TR.transcribe(model, audio[16000:88000], **KW)
    assert len(group.verifies) == n + 2 and mem.dropped == 1
    assert TR.transcribe(model, audio[16000:96000], draft=mem, **KW) == TR.transcribe(model, audio[16000:96000], **KW)
    assert len(group.verifies) == n + 3                                           # the refreshed memory serves again
    TR.release_sessions(model)


def test_only_the_first_window_at_the_first_temperature_sees_the_draft(real_vocab, model, monkeypatch):
    group = _with_stack(model, monkeypatch)
    seen = []
    real_run = TR._WindowDecoder.run

    def run(self, *a, **k):
        seen.append((self.o.temperature, self.o.beam_size, None if self.o.draft is None else list(self.o.draft)))
        return real_run(self, *a, **k)
    monkeypatch.setattr(TR._WindowDecoder, "run", run)
    audio = synth.speech_like(40.0, seed=6)                   # two windows
    mem = TR.WindowDraft()
    mem.begin(audio[:1000])
    mem.remember([600, 601, 602, 603, 604, 605, 606, 607])
    # every result misses the log-probability threshold: the whole ladder runs for both windows
    kw = dict(KW, temperature=(0.0, 0.4), logprob_threshold=0.0)
    TR.transcribe(model, audio, draft=mem, **kw)
    assert [s[0] for s in seen] == [0.0, 0.4, 0.0, 0.4]
    assert seen[0][2] == [600, 601, 602, 603, 604, 605, 606, 607] and all(s[2] is None for s in seen[1:])
    # a ladder that does not start at 0, and beam search, never see it
    for extra in (dict(temperature=(0.4,)), dict(temperature=0.0, beam_size=2)):
        del seen[:]
        mem.begin(audio[:1000])
        mem.remember([600, 601, 602])
        TR.transcribe(model, audio, draft=mem, **dict(KW, **extra))
        assert seen and all(s[2] is None for s in seen), seen
    TR.release_sessions(model)


# ---- 5. the switch and the per-session view -----------------------------------------------------------------------------------
def test_the_draft_switch_needs_the_stack_and_the_argument_wins(real_vocab, model, monkeypatch):
    assert TR.resolve_draft(None) is False and TR.resolve_draft(True) is True
    monkeypatch.setenv("WLK_TRANSCRIBE_DRAFT", "1")
    assert TR.resolve_draft(None) is True and TR.resolve_draft(False) is False
    with pytest.raises(ValueError):
        LA.HipWhisperASR("en", hip_model=model, stack=0, draft=True)
    assert LA.HipWhisperASR("en", hip_model=model, stack=0).draft is False        # the environment alone: off without a stack
    assert LA.HipWhisperASR("en", hip_model=model, stack=2).draft is True
    assert LA.HipWhisperASR("en", hip_model=model, stack=2, draft=False).draft is False
    monkeypatch.delenv("WLK_TRANSCRIBE_DRAFT")
    assert LA.HipWhisperASR("en", hip_model=model, stack=2).draft is False
    assert LA.HipWhisperASR("en", hip_model=model, stack=2, draft=True).draft is True
    TR.set_stack(model, 0)


def test_session_views_share_the_model_and_own_their_memory(real_vocab, model, monkeypatch):
    group = _with_stack(model, monkeypatch)
    asr = LA.HipWhisperASR("en", hip_model=model, stack=8, draft=True)
    asr.transcribe_kargs = {k: v for k, v in KW.items() if k != "language"}
    a, b = asr.session_view(), asr.session_view()
    assert a.memory is not None and a.memory is not b.memory and a.model is asr.model is b.model
    # what the reference's backend_factory sets afterwards lands in the shared object and reads back through every view
    for name, value in (("tokenizer", object()), ("confidence_validation", True), ("buffer_trimming", "sentence"),
                        ("buffer_trimming_sec", 9), ("backend_choice", "whisper")):
        setattr(a, name, value)
        assert getattr(asr, name) is value and getattr(b, name) is value
    assert a.sep == asr.sep and a.original_language == "en"
    for name in ("transcribe", "ts_words", "segments_end_ts", "use_vad"):
        assert callable(getattr(a, name))
    audio = synth.speech_like(6.0, seed=5)
    want = asr.transcribe(audio[:64000])
    assert group.verifies == []                               # without a view, transcribe is the call it was
    assert a.transcribe(audio[:64000]) == want and group.verifies == []
    assert b.memory.audio is None and len(a.memory.tokens) == 12
    assert a.transcribe(audio[:72000]) == asr.transcribe(audio[:72000]) and len(group.verifies) == 1
    assert b.transcribe(audio[:72000]) == asr.transcribe(audio[:72000]) and len(group.verifies) == 1     # b's first call
    assert a.ts_words(want) == asr.ts_words(want) and a.segments_end_ts(want) == asr.segments_end_ts(want)
    off = LA.HipWhisperASR("en", hip_model=model, stack=8)
    assert off.session_view().memory is None
    TR.set_stack(model, 0)
    TR.release_sessions(model)


# ---- 6. the GPU tests' windows ------------------------------------------------------------------------------------------------
def test_the_verify_windows_keep_their_decisions_clear_of_rounding(real_vocab):
    """At every step of the windows of tests/draft_verify_cases.py the oracle's best allowed token leads the runner-up by
    >= 1e-3 in log-probability, and the timestamps-against-text decision is as far from flipping, so the GPU file compares
    token ids without a tie escape; the windows end the way that file relies on."""
    model = WG.PickingOracleModel(DV.MODEL, DV.SEED)
    wins, walked = [], set()
    for i, spec in enumerate(DV.WINDOWS):
        w = DV.make_win(i, model, model.new_session())
        s = w.session
        s.encode_mel(TR.pad_or_trim(s.log_mel(WG.window_audio(spec))))
        s.set_rules(*w.rules())
        s.decode(w.tokens, first=True, sot_index=w.dec.sot_index)
        state = w.dec._pick_state(w.tokens)
        w.take(*s.pick_greedy(**state), s.margins[-1])
        while not w.over:
            nxt = TR._next_pick_state(state, w.picks[-1][0])
            if i in DV.TS_WINDOWS:
                walked.add((state["ts_mode"], nxt["ts_mode"]))
            state = nxt
            s.decode(w.tokens[:, -1:], first=False)
            w.take(*s.pick_greedy(**state), s.margins[-1])
        wins.append(w)
    print("steps per window:", [len(w.picks) for w in wins], f"worst margin {min(m for w in wins for m in w.extra):.3e}")
    for w in wins:
        assert min(w.extra) >= DV.MARGIN, (w.index, [f"{m:.2e}" for m in w.extra])
    assert {(0, 1), (1, 0), (0, 2), (2, 1)} <= walked, walked
    eot = wins[0].dec.tok.eot
    e = wins[DV.EOT_WINDOW]
    assert e.picks[-1][0] == eot and len(e.picks) == 2
    assert len(e.dec.initial) + len(e.picks) - 1 + 3 >= 9                        # its draft plus three tokens rides the pass
    assert all(w.picks[-1][0] != eot and len(w.picks) == w.spec["sample_len"] for w in wins if w is not e)
    assert [len(w.dec.initial) for w in wins] == [1, 2, 7, 12, 1] and wins[DV.PROMPT_WINDOW].dec.sot_index == 6
