"""Beam search inside the library decode loop (wlk_decode_beam_until_stop, beams 2-7), host half, without a GPU:
wlk_beam_job_* against policy.BeamUpdate on seeded inputs, the reference's beam golden streams through the loop
(tests/beam_loop_standin.py: the library's host logic over the oracle's numerics), and the opt-in switch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import helpers as H
from beam_loop_standin import BeamLoopFakeModel
from test_oracle_golden import replay_stream
from test_policy_golden import check_loop_stream
from whisperlivekit_amd import _lib, policy as P, tokenizer as T
from whisperlivekit_amd.backend import HipSimulStreamingASR, HipSimulStreamingOnlineProcessor
from whisperlivekit_amd.dims import ALIGNMENT_HEADS, MODEL_DIMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOT = 50256
NEW_SYMBOLS = ["wlk_decode_beam_until_stop", "wlk_session_beam_stats", "wlk_diag_beam_step", "wlk_beam_job_create",
               "wlk_beam_job_begin_step", "wlk_beam_job_no_speech", "wlk_beam_job_adjustments", "wlk_beam_job_consume",
               "wlk_beam_job_state", "wlk_beam_job_result", "wlk_beam_job_destroy"]


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def quiet_params(**over):
    """Loop parameters under which no stop rule but `completed` can fire, so every update of a case is compared."""
    kw = dict(sot_index=0, is_last=0, frame_threshold=-10 ** 6, rewind_threshold=10 ** 6, last_attend_frame=0,
              max_text_len=10 ** 6, budget=10 ** 6, eot=EOT, dec_pad=P.DEC_PAD, no_speech_token=-1,
              no_speech_threshold=0.5, content_mel_len=1500)
    kw.update(over)
    return _lib.LoopParams(**kw)


def job_state(lib, job, B, n):
    rows, sums, src = np.empty((B, n), np.int64), np.empty(B, np.float32), np.empty(B, np.int32)
    n_len, done = C.c_int32(), C.c_int32()
    _lib.check(lib.wlk_beam_job_state(job, vp(rows), rows.size, C.byref(n_len), vp(sums), vp(src), C.byref(done)))
    assert n_len.value == n
    return rows, sums, src, bool(done.value)


def candidates(rng, B, mode, p_eot):
    """[B][B + 1] (log-prob, id): distinct ids per row, log-probs descending.  `dyadic`: quarter steps, so sums of
    different rows meet exactly and the stable ranking / dict order decides; `shared`: every row has the same list
    (what identical rows produce on the first step)."""
    K = B + 1
    lp, ids = np.empty((B, K), np.float32), np.empty((B, K), np.int32)
    for b in range(B):
        pool = rng.choice(np.arange(300, 300 + 3 * K), size=K, replace=False)
        if rng.random() < p_eot:
            pool[rng.integers(0, K)] = EOT
        ids[b] = pool
        vals = -rng.integers(0, 6, K) / 4.0 if mode == "dyadic" else -rng.random(K) * 4.0
        lp[b] = np.sort(vals.astype(np.float32))[::-1]
    if mode == "shared":
        lp[:], ids[:] = lp[0], ids[0]
    return lp, ids


@pytest.mark.parametrize("B", [2, 3, 5, 7])
@pytest.mark.parametrize("mode", ["dyadic", "random", "shared"])
def test_beam_job_update_equals_policy_beam_update(B, mode):
    """New tokens, source rows, `completed` and sum_logprobs (bitwise) of every update: identical rows on the first step,
    exactly equal scores (dyadic log-probs), end-of-text among the candidates, `finished` filling over several steps."""
    lib = _lib.load()
    steps_seen = eot_steps = tie_steps = multi_step_fill = 0
    for seed in range(40):
        rng = np.random.default_rng(1000 * B + seed)
        prompt = np.array([50257, 50362] + rng.integers(300, 330, 3).tolist(), np.int64)
        params = quiet_params()
        job = C.c_void_p()
        _lib.check(lib.wlk_beam_job_create(C.byref(params), B, vp(prompt), prompt.size, None, 0, None, 0, C.byref(job)))
        try:
            upd = P.BeamUpdate(B, EOT)
            tokens = np.tile(prompt, (B, 1))
            sums = np.zeros(B, np.float32)
            fills = []
            for step in range(14):
                n_feed = C.c_int32()
                _lib.check(lib.wlk_beam_job_begin_step(job, C.byref(n_feed)))
                assert n_feed.value == (prompt.size if step == 0 else 1)
                lp, ids = candidates(rng, B, "shared" if (mode == "shared" and step == 0) else
                                     ("dyadic" if mode == "shared" else mode), p_eot=0.35)
                scores = (sums[:, None] + lp).ravel()
                tie_steps += int(len(np.unique(scores)) < scores.size)
                eot_steps += int((ids == EOT).any())
                want_tokens, want_done, want_src = upd.update(tokens, lp, ids, sums)
                go = C.c_int32()
                frames = np.zeros(B, np.int32)
                _lib.check(lib.wlk_beam_job_consume(job, vp(lp), vp(ids), vp(frames), C.byref(go)))
                rows, got_sums, src, done = job_state(lib, job, B, tokens.shape[1] + 1)
                assert rows.tolist() == want_tokens.tolist(), (seed, step)
                assert src.tolist() == list(want_src), (seed, step)
                assert done == want_done and bool(go.value) == (not want_done), (seed, step)
                assert got_sums.view(np.uint32).tolist() == sums.view(np.uint32).tolist(), (seed, step)
                tokens = want_tokens
                fills.append(len(upd.finished[0]))
                steps_seen += 1
                if want_done:
                    res = _lib.LoopResult()
                    new = np.empty(64, np.int64)
                    _lib.check(lib.wlk_beam_job_result(job, C.byref(res), vp(new), None, None, None, 64))
                    assert res.stop_reason == _lib.STOP_COMPLETED and res.n_steps == step + 1
                    assert new[:res.n_new_tokens].tolist() == tokens[0, prompt.size:-1].tolist()
                    assert np.float32(res.sum_logprob).view(np.uint32) == sums[:1].view(np.uint32)[0]
                    break
            multi_step_fill += int(len({f for f in fills if 0 < f < B}) > 0 and fills[-1] >= B)
        finally:
            lib.wlk_beam_job_destroy(job)
    assert steps_seen > 80 and eot_steps > 20 and multi_step_fill > 0
    if mode != "random":
        assert tie_steps > 20


def test_beam_job_stop_rules_follow_row_zero():
    """budget, context, frame threshold and rewind as policy._decode_loop applies them to row 0."""
    lib = _lib.load()
    B = 3
    prompt = np.array([50257, 50362, 400, 401], np.int64)

    def run(params, frames_per_step, n_steps=6):
        job = C.c_void_p()
        _lib.check(lib.wlk_beam_job_create(C.byref(params), B, vp(prompt), prompt.size, None, 0, None, 0, C.byref(job)))
        try:
            rng = np.random.default_rng(5)
            for step in range(n_steps):
                n_feed = C.c_int32()
                _lib.check(lib.wlk_beam_job_begin_step(job, C.byref(n_feed)))
                if n_feed.value == 0:
                    break
                lp, ids = candidates(rng, B, "random", p_eot=0.0)
                go = C.c_int32()
                fr = np.full(B, frames_per_step[min(step, len(frames_per_step) - 1)], np.int32)
                fr[1:] += 7                       # only row 0's frame may matter
                _lib.check(lib.wlk_beam_job_consume(job, vp(lp), vp(ids), vp(fr), C.byref(go)))
                if not go.value:
                    break
            res = _lib.LoopResult()
            new, sf = np.empty(64, np.int64), np.empty(64, np.int32)
            _lib.check(lib.wlk_beam_job_result(job, C.byref(res), vp(new), None, vp(sf), None, 64))
            return res, sf[:res.n_steps].tolist()
        finally:
            lib.wlk_beam_job_destroy(job)

    res, sf = run(quiet_params(frame_threshold=4, content_mel_len=100), [10, 20, 97])
    assert (res.stop_reason, res.n_steps, res.n_new_tokens, res.last_attend_frame, sf) == (_lib.STOP_FRAME, 3, 2, 97, [10, 20, 97])
    res, _ = run(quiet_params(rewind_threshold=50, last_attend_frame=300), [10])
    assert (res.stop_reason, res.n_steps, res.n_new_tokens, res.last_attend_frame) == (_lib.STOP_REWIND, 1, 0, -50)
    res, _ = run(quiet_params(budget=2), [10])
    assert (res.stop_reason, res.n_steps, res.n_new_tokens, res.decode_calls) == (_lib.STOP_BUDGET, 2, 0, 2)
    res, _ = run(quiet_params(max_text_len=prompt.size + 3), [10])
    assert (res.stop_reason, res.n_steps, res.n_new_tokens) == (_lib.STOP_CONTEXT_FULL, 3, 3)


# ---- the reference's beam golden streams through the loop ---------------------------------------------------------------
def make_beam_loop_processor(model_name, cfg_over, seed=0):
    dims = MODEL_DIMS[model_name]
    fake = BeamLoopFakeModel(dims, H.oracle_sd(model_name, seed), ALIGNMENT_HEADS[model_name])
    asr = HipSimulStreamingASR(model_name, hip_model=fake, **H.asr_kwargs(cfg_over))

    class P2(HipSimulStreamingOnlineProcessor):
        def new_speaker(self, speaker, start):
            return super().new_speaker(P.ChangeSpeaker(speaker=speaker, start=start))

    proc = P2(asr)
    proc.model.decision_log = []
    proc.model.use_beam_loop = True
    assert proc.model.beam_loop_available() and not proc.model.device_loop_available()
    return proc


@pytest.fixture
def real_vocab(tmp_path, monkeypatch):
    d = H.real_vocab_dir(tmp_path)
    monkeypatch.delenv("WLK_SYNTHETIC_VOCAB", raising=False)
    monkeypatch.setenv("WLK_VOCAB_DIR", d)
    T.get_encoding.cache_clear()
    T._get_tokenizer.cache_clear()
    yield d
    T.get_encoding.cache_clear()
    T._get_tokenizer.cache_clear()


def check_beam_stream(case):
    g, proc, got = replay_stream(case, make_beam_loop_processor)
    assert proc.model.cfg.beam_size == g["cfg"]["beam_size"] >= 2
    r = check_loop_stream(g, proc, got)
    assert r["calls"] == len(g["calls"]) and r["decisions"] > 0
    return proc


@pytest.mark.parametrize("case", ["micro_beam2", "micro_minlen_beam3"])
def test_beam_golden_stream_through_the_library_loop(case):
    check_beam_stream(case)


def test_beam_golden_stream_through_the_library_loop_on_real_vocabulary(real_vocab):
    proc = check_beam_stream("micro_realvocab_beam2")
    assert isinstance(proc.model.tokenizer.encoding, T.BpeEncoding)


# ---- the switch -----------------------------------------------------------------------------------------------------------
def hooks(monkeypatch=None, **kw):
    fake = BeamLoopFakeModel(MODEL_DIMS["micro.en"], H.oracle_sd("micro.en", 0), ALIGNMENT_HEADS["micro.en"])
    asr = HipSimulStreamingASR("micro.en", hip_model=fake, **kw)
    return HipSimulStreamingOnlineProcessor(asr).model


def test_beam_loop_switch(monkeypatch):
    monkeypatch.delenv("WLK_BEAM_LOOP", raising=False)
    m = hooks(beams=3)
    assert not m.beam_loop_available()                       # off by default
    assert not m.device_loop_available()                     # keeps its beam-1 meaning
    m.use_beam_loop = True
    assert m.beam_loop_available()
    m.teacher = {(0, 0): (1, 1)}
    assert not m.beam_loop_available()
    m.teacher = None
    m.use_beam_loop = False
    monkeypatch.setenv("WLK_BEAM_LOOP", "1")
    assert m.beam_loop_available()
    assert not hooks(beams=1).beam_loop_available()
    assert hooks(beams=1).device_loop_available()
    assert not hooks(beams=3, decoder_type="greedy").beam_loop_available()
    assert hooks(beams=7).beam_loop_available()
    m8 = hooks(beams=2)
    m8.cfg.beam_size = 8
    assert not m8.beam_loop_available()
    plain = hooks(beams=2)
    from fake_session import FakeSession
    plain.session = FakeSession(plain.model, 2)             # a session without the method
    assert not plain.beam_loop_available()


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "wlk_hip.h")).read()
    declared = set(re.findall(r"\b(wlk_[a-z_0-9]+)\s*\(", header))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "wlk_decode_beam_until_stop" in integration
    from whisperlivekit_amd.engine import HipSession
    assert hasattr(HipSession, "decode_beam_until_stop")
