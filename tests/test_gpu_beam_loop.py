"""Beam search inside the library decode loop on the GPU (wlk_decode_beam_until_stop, beams 2-7): the reference's beam
golden streams through the real library, the loop against the per-token path on the same seeded model and audio, the
ancestry self-attention against cache gather + the plain kernel (bitwise), the state guard and the fallback."""
import json
import os

import numpy as np
import pytest

import helpers as H
from whisperlivekit_amd import _lib, policy as P, synth, tokenizer as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}
_models = {}


def report(key, **vals):
    """Figures of a test: printed, and kept as beam_loop_report.json where WLK_REPORT_DIR names a directory."""
    REPORT[key] = vals
    print(f"[beam loop] {key}: {json.dumps(vals, sort_keys=True, default=str)}")
    out = os.environ.get("WLK_REPORT_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "beam_loop_report.json"), "w") as fh:
            json.dump(REPORT, fh, indent=1, sort_keys=True, default=str)


def hip_model(name, seed=0):
    from whisperlivekit_amd.engine import HipWhisperModel
    if (name, seed) not in _models:
        assert _lib.load().wlk_device_count() > 0, "no MI355X visible"
        _models[(name, seed)] = HipWhisperModel.synthetic(name, seed)
    return _models[(name, seed)]


def make_processor(model_name, cfg_over, seed=0, loop=True, debug=False):
    from whisperlivekit_amd.backend import HipSimulStreamingASR, HipSimulStreamingOnlineProcessor
    asr = HipSimulStreamingASR(model_name, hip_model=hip_model(model_name, seed), **H.asr_kwargs(cfg_over))

    class P2(HipSimulStreamingOnlineProcessor):
        def new_speaker(self, speaker, start):
            return super().new_speaker(P.ChangeSpeaker(speaker=speaker, start=start))

    proc = P2(asr)
    proc.model.decision_log = []
    proc.model.use_beam_loop = loop
    assert proc.model.beam_loop_available() == loop
    if debug:
        proc.model.session.set_debug(True)
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


def golden_through_loop(case, **kw):
    from test_oracle_golden import replay_stream
    from test_policy_golden import check_loop_stream
    g, proc, got = replay_stream(case, lambda m, c, s=0: make_processor(m, c, s, **kw))
    try:
        emitted = [[(t.start, t.end, t.text) for t in toks] for ev, toks, _ in got if ev["kind"] == "chunk"]
        r = H.compare_decisions(g, proc.model.decision_log, emitted)
        stats = proc.model.session.beam_stats()
        report(f"golden_{case}_{'debug' if kw.get('debug') else 'loop'}", **r, forced_decisions=0, **stats)
        assert r["mismatch"] is None and r["tie_divergence"] is None, r       # zero forced decisions
        assert r["calls"] == len(g["calls"]) and r["identical"] == r["decisions"] > 0 and r["words_identical"], r
        check_loop_stream(g, proc, got)
        return stats
    finally:
        proc.close()


@pytest.mark.parametrize("case", ["micro_beam2", "micro_minlen_beam3"])
def test_beam_golden_stream_through_the_library_loop(case):
    """micro.en (d = 128, two 64-wide heads) is a shape the <= 8-row weight-streaming kernels take, so these streams run
    their single-token steps over the ancestry table; the fallback is covered by the debug sessions below."""
    assert golden_through_loop(case)["ancestry_steps"] > 0


def test_beam_golden_stream_through_the_library_loop_on_real_vocabulary(real_vocab):
    assert golden_through_loop("micro_realvocab_beam2")["ancestry_steps"] > 0


def test_debug_session_completes_the_loop_through_the_fallback():
    """set_debug(1) disqualifies the ancestry step: every step runs as wlk_decode + wlk_select + wlk_kv_reorder inside the
    call; same decisions as the reference."""
    stats = golden_through_loop("micro_beam2", debug=True)
    assert stats["ancestry_steps"] == 0


# ---- loop against the per-token path -------------------------------------------------------------------------------------
def run_stream(model_name, beams, seconds, audio_seed, loop, debug=False):
    proc = make_processor(model_name, dict(beam_size=beams), loop=loop, debug=debug)
    m = proc.model
    sums, outcomes, stops = [], [], []
    if loop:
        orig = m.session.decode_beam_until_stop

        def wrapped(*a):
            out = orig(*a)
            outcomes.append(out)
            stops.append(out.stop_reason)
            sums.append([np.float32(x).view(np.uint32).item() for x in out.step_sum_logprobs])
            return out
        m.session.decode_beam_until_stop = wrapped
    else:
        # the per-token loop (policy._decode_loop) names no stop reason: it is read off what the loop did last
        upd0, enc0, ns0, rew0, infer0 = m._update_tokens, m._encode, m._check_no_speech, m._rewind_tokens, m.infer
        seen = {}

        def _enc(segs):
            sums.append([])
            seen.clear()
            seen["encoded"] = True
            return enc0(segs)

        def _ns(logits):
            seen["no_speech"] = ns0(logits)
            return seen["no_speech"]

        def _upd(tokens, logits, slp):
            r = upd0(tokens, logits, slp)
            sums[-1].append(np.float32(slp[0]).view(np.uint32).item())
            seen.update(done=bool(r[1]), n_tok=int(r[0].shape[1]), frame=int(m._last_frames[0]), steps=seen.get("steps", 0) + 1)
            return r

        def _rew():
            seen["rewound"] = True
            return rew0()

        def _infer(is_last=False):
            seen.clear()
            out = infer0(is_last=is_last)
            if seen.get("encoded"):
                thr = 4 if is_last else m.cfg.frame_threshold
                if seen.get("no_speech"):
                    stops.append(_lib.STOP_NO_SPEECH)
                elif not seen.get("steps"):
                    stops.append(_lib.STOP_CONTEXT_FULL)
                elif seen["done"]:
                    stops.append(_lib.STOP_COMPLETED)
                elif seen.get("rewound"):
                    stops.append(_lib.STOP_REWIND)
                elif m._content_mel_len - seen["frame"] <= thr:
                    stops.append(_lib.STOP_FRAME)
                elif seen["n_tok"] >= m.max_text_len:
                    stops.append(_lib.STOP_CONTEXT_FULL)
                else:
                    stops.append(_lib.STOP_BUDGET)
            return out
        m._update_tokens, m._encode, m._check_no_speech, m._rewind_tokens, m.infer = _upd, _enc, _ns, _rew, _infer
    try:
        audio = synth.to_pcm16_roundtrip(synth.speech_like(seconds, audio_seed))
        words, hyps, last_attend = [], [], []
        for lo in range(0, len(audio), 8000):
            hi = min(lo + 8000, len(audio))
            proc.insert_audio_chunk(audio[lo:hi].copy(), hi / 16000)
            toks, _ = proc.process_iter()
            words.append([(t.start, t.end, t.text) for t in toks])
            hyps.append([t[0].tolist() for t in m.state.tokens[1:]])
            last_attend.append(m.state.last_attend_frame)
        return dict(decisions=[[c, [(int(t), int(f)) for t, f in s]] for c, s in m.decision_log], words=words, hyps=hyps,
                    last_attend=last_attend, sums=[s for s in sums], context=m.state.context.text,
                    stops=stops, ancestry_steps=m.session.beam_stats()["ancestry_steps"])
    finally:
        proc.close()


@pytest.mark.parametrize("model_name,beams,seconds", [("base.en", 2, 6.0), ("base.en", 3, 6.0), ("base.en", 5, 6.0),
                                                      ("tiny.en", 7, 3.0)])
def test_loop_equals_per_token_path(model_name, beams, seconds):
    """Same seeded model and audio: per-step tokens, frames, sum_logprobs (bitwise: the loop runs the per-token path's
    kernels, the ancestry self-attention keeps the plain kernel's arithmetic), committed words and end state."""
    a = run_stream(model_name, beams, seconds, 11, loop=True)
    b = run_stream(model_name, beams, seconds, 11, loop=False)
    n_steps = sum(len(s) for _, s in b["decisions"])
    report(f"loop_vs_per_token_{model_name}_beam{beams}", steps=n_steps, ancestry_steps=a["ancestry_steps"],
           decisions_equal=a["decisions"] == b["decisions"], sums_bitwise_equal=a["sums"] == b["sums"],
           stops=a["stops"], stops_per_token=b["stops"])
    assert n_steps > 10
    assert a["decisions"] == b["decisions"]
    assert a["stops"] == b["stops"] and len(a["stops"]) == len(a["decisions"])
    assert a["sums"] == b["sums"]
    assert a["words"] == b["words"] and a["hyps"] == b["hyps"]
    assert a["last_attend"] == b["last_attend"] and a["context"] == b["context"]
    assert a["ancestry_steps"] > 0 and b["ancestry_steps"] == 0     # the graph-replayed ancestry step really ran


def test_fallback_on_a_shape_that_would_qualify():
    """tiny.en qualifies for the ancestry step; with set_debug(1) the loop runs every step as wlk_kv_reorder + wlk_decode
    + wlk_select inside the call.  Against the per-token path of a debug session (same kernels): the same stream."""
    a = run_stream("tiny.en", 3, 3.0, 21, loop=True, debug=True)
    b = run_stream("tiny.en", 3, 3.0, 21, loop=False, debug=True)
    assert a["ancestry_steps"] == 0 and sum(len(s) for _, s in a["decisions"]) > 10
    for k in ("decisions", "sums", "stops", "words", "hyps", "last_attend", "context"):
        assert a[k] == b[k], k


# ---- ancestry attention against gather + the plain kernel --------------------------------------------------------------------
def prefilled_pair(model_name, beam, n_prompt=7):
    model = hip_model(model_name)
    audio = synth.speech_like(3.0, 4)
    rng = np.random.default_rng(beam)
    prompt = np.tile(np.array([[50257, 50362] + rng.integers(300, 40000, n_prompt - 2).tolist()], np.int64), (beam, 1))
    pair = []
    for _ in range(2):
        s = model.new_session(beam=beam)
        s.append(audio)
        s.encode()
        s.decode(prompt, first=True, sot_index=0)
        pair.append(s)
    return pair, rng, prompt


@pytest.mark.parametrize("model_name,beam", [("tiny.en", 5), ("base.en", 7), ("base.en", 2)])
def test_ancestry_attention_equals_gather_and_plain_kernel(model_name, beam):
    (ref, anc), rng, _ = prefilled_pair(model_name, beam)
    try:
        V = hip_model(model_name).dims.n_vocab
        worst = 0
        for step in range(24):
            if step % 6 == 0:
                src = np.arange(beam)                                 # identity
            elif step % 6 == 1:
                src = np.full(beam, rng.integers(0, beam))            # one ancestor shared by all, the rest dropped
            else:
                src = np.sort(rng.integers(0, beam, beam))            # shared and dropped ancestors
                if step % 2:
                    src = src[::-1].copy()
            tokens = rng.integers(300, 40000, (beam, 1)).astype(np.int64)
            ref.kv_reorder(src.tolist())
            ref.decode(tokens, first=False)
            anc.beam_step(tokens[:, 0], src)
            want = ref.export("logits_last", beam * V).view(np.uint32)
            got = anc.export("logits_last", beam * V).view(np.uint32)
            worst = max(worst, int((want != got).sum()))
            assert worst == 0, (step, src.tolist())
        assert anc.beam_stats()["ancestry_steps"] == 24 and ref.beam_stats()["ancestry_steps"] == 0
        report(f"ancestry_attention_{model_name}_beam{beam}", steps=24, differing_logits=worst)
    finally:
        ref.close()
        anc.close()


def test_ancestry_steps_after_a_reorder_in_an_earlier_infer():
    """wlk_kv_reorder flips the session's KV buffer; the captured ancestry step is kept per buffer.  An infer that ran
    through the gather path (debug / profiling fallback, per-token hooks), then infers over the ancestry table on either
    buffer: logits_last bitwise equal to the gather path after every step."""
    beam = 3
    (ref, anc), rng, prompt = prefilled_pair("tiny.en", beam)
    try:
        V = hip_model("tiny.en").dims.n_vocab

        def gather_step(sess):
            tokens = rng.integers(300, 40000, (beam, 1)).astype(np.int64)
            sess.kv_reorder([2, 0, 0])
            sess.decode(tokens, first=False)

        def compare_infer(n, prefill=True):
            for sess in (ref, anc) if prefill else ():
                sess.decode(prompt, first=True, sot_index=0)
            for step in range(n):
                src = np.array([[1, 1, 0], [0, 2, 2], [2, 1, 0], [0, 1, 2]][step % 4])
                tokens = rng.integers(300, 40000, (beam, 1)).astype(np.int64)
                ref.kv_reorder(src.tolist())
                ref.decode(tokens, first=False)
                anc.beam_step(tokens[:, 0], src)
                want = ref.export("logits_last", beam * V).view(np.uint32)
                got = anc.export("logits_last", beam * V).view(np.uint32)
                assert (want == got).all(), (step, src.tolist())

        compare_infer(6)                      # captures the ancestry step on buffer 0
        anc.decode(prompt, first=True, sot_index=0)
        gather_step(anc)                      # an infer through the gather path: buffer 1 from here on
        compare_infer(6)                      # ancestry steps on buffer 1
        anc.decode(prompt, first=True, sot_index=0)
        gather_step(anc)                      # back to buffer 0
        compare_infer(6)
        tokens = rng.integers(300, 40000, (beam, 1)).astype(np.int64)
        for sess in (ref, anc):               # a reorder and then ancestry steps in the SAME infer (fresh table)
            sess.decode(prompt, first=True, sot_index=0)
            sess.kv_reorder([1, 2, 2])
            sess.decode(tokens, first=False)
        compare_infer(5, prefill=False)
    finally:
        ref.close()
        anc.close()


def test_state_guard_after_an_ancestry_step():
    (plain, s), rng, prompt = prefilled_pair("tiny.en", 3)
    try:
        tokens = rng.integers(300, 40000, (3, 1)).astype(np.int64)
        s.beam_step(tokens[:, 0], [1, 1, 0])
        with pytest.raises(_lib.WlkError, match=r"error -3"):
            s.kv_reorder([0, 0, 1])
        with pytest.raises(_lib.WlkError, match=r"error -3"):
            s.kv_reorder([0, 1, 2])
        with pytest.raises(_lib.WlkError, match=r"error -3"):
            s.decode(tokens, first=False)
        s.decode(prompt, first=True, sot_index=0)                    # the next infer works, on either path
        plain.decode(prompt, first=True, sot_index=0)
        for sess in (s, plain):
            sess.kv_reorder([2, 0, 0])
            sess.decode(tokens, first=False)
        V = hip_model("tiny.en").dims.n_vocab
        assert (s.export("logits_last", 3 * V).view(np.uint32) == plain.export("logits_last", 3 * V).view(np.uint32)).all()
    finally:
        plain.close()
        s.close()
