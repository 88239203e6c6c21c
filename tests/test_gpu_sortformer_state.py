"""Device-resident Sortformer sessions (wlk_sf_session_*): the state kernels of csrc/sortformer_state.hip against the numpy
restatement sortformer.streaming_update / compress_spkcache (itself pinned to the oracle by tests/test_sortformer_host.py),
bit for bit; the whole session on the device against the host-state path; stacking with host sessions; the ABI contract.

The one allowed difference: logf on the device and numpy's log may differ by an ulp, which can only matter where two
scores of the compression are closer than that at a top-k cut.  Where the host's scores have such a near-tie (gap < 1e-5)
the speaker cache may be selected differently; the tests detect it on the host side, re-synchronise and count it."""
import copy
import math
import threading

import numpy as np
import pytest

from whisperlivekit_amd import _lib
from whisperlivekit_amd import sortformer as sf
from whisperlivekit_amd.diarization import HipMelSpectrogram, HipSortformerDiarizationOnline
from whisperlivekit_amd.synth import speech_like

pytestmark = pytest.mark.gpu

NEAR = 1e-5


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def beq(a, b):
    return np.array_equal(bits(a), bits(b))


def cut_gap(sp, preds):
    """Smallest gap between finite scores on either side of any top-k cut of compress_spkcache (host arithmetic)."""
    n_frames, n_spk = preds.shape
    per_spk = sp.spkcache_len // n_spk - sp.spkcache_sil_frames_per_spk
    strong, weak = math.floor(per_spk * sp.strong_boost_rate), math.floor(per_spk * sp.weak_boost_rate)
    min_pos = math.floor(per_spk * sp.min_pos_scores_rate)
    thr = np.float32(sp.pred_score_threshold)
    log_p = np.log(np.maximum(preds, thr))
    log_1p = np.log(np.maximum(np.float32(1.0) - preds, thr))
    scores = (log_p - log_1p + log_1p.sum(axis=1, keepdims=True) - np.float32(math.log(0.5))).astype(np.float32)
    is_speech = preds > 0.5
    scores = np.where(is_speech, scores, -np.inf).astype(np.float32)
    is_pos = scores > 0
    scores = np.where((~is_pos) & is_speech & (is_pos.sum(axis=0, keepdims=True) >= min_pos), -np.inf, scores).astype(np.float32)
    if sp.scores_boost_latest > 0:
        scores[sp.spkcache_len:, :] += np.float32(sp.scores_boost_latest)
    gap = np.inf

    def at_cut(v, k):
        s = np.sort(v[np.isfinite(v)])[::-1]
        n_inf = int(np.sum(v == np.inf))
        k = k - n_inf
        if 0 < k < len(s):
            return float(s[k - 1] - s[k])
        return np.inf

    for n_boost, factor in ((strong, 2.0), (weak, 1.0)):
        for s in range(n_spk):
            gap = min(gap, at_cut(scores[:, s], min(n_boost, n_frames)))
            idx = np.argsort(-scores[:, s], kind="stable")[: min(n_boost, n_frames)]
            scores[idx, s] -= np.float32(factor * math.log(0.5))
    return min(gap, at_cut(scores.T.reshape(-1), sp.spkcache_len))


class CompressRecorder:
    """Wraps sortformer.compress_spkcache (streaming_update calls it by module name) to record each call's cut gap."""

    def __init__(self, monkeypatch):
        self.gaps = []
        orig = sf.compress_spkcache

        def rec(sp, emb, preds, mean):
            self.gaps.append(cut_gap(sp, preds))
            return orig(sp, emb, preds, mean)
        monkeypatch.setattr(sf, "compress_spkcache", rec)


def assert_state_rule1(host, dev, recorder_gaps_before, recorder):
    """Rule 1: lengths, FIFO, its activities, the silence profile bitwise; the speaker cache bitwise unless this step's
    compression had a near-tie.  -> True when the cache differed at a near-tie (the caller re-synchronises)."""
    assert (host.spkcache_len, host.fifo_len, host.n_sil_frames) == (dev.spkcache_len, dev.fifo_len, dev.n_sil_frames)
    for name in ("fifo", "fifo_preds", "mean_sil_emb"):
        assert beq(getattr(host, name), getattr(dev, name)), name
    same = beq(host.spkcache, dev.spkcache) and beq(host.spkcache_preds, dev.spkcache_preds)
    if same:
        return False
    new_gaps = recorder.gaps[recorder_gaps_before:]
    assert new_gaps and min(new_gaps) < NEAR, f"speaker cache differs without a near-tie (gaps {new_gaps})"
    return True


@pytest.fixture(scope="module")
def small():
    dims = sf.SortformerDims(fc_layers=1, tf_layers=1)
    m = sf.HipSortformerModel(dims, sf.synth_sortformer_state_dict(dims, 21))
    yield m
    m.close()


@pytest.fixture(scope="module")
def full():
    dims = sf.SortformerDims()
    m = sf.HipSortformerModel(dims, sf.synth_sortformer_state_dict(dims, 12))
    yield m
    m.close()


def random_stream(seed, n_steps, d=512):
    rng = np.random.default_rng(seed)
    for step in range(n_steps):
        tc = 13 if step == 0 else 25
        yield step, rng.standard_normal((tc, d)).astype(np.float32), rng


@pytest.mark.parametrize("seed,silence", [(0, False), (1, True), (2, False), (3, True)])
def test_update_kernels_equal_numpy_streaming_update(small, monkeypatch, seed, silence):
    m, sp = small, small.cache
    rec = CompressRecorder(monkeypatch)
    host = m.new_state() if not m.device_state else None
    if host is None:
        pytest.fail("the fixture model must default to host state")
    dev = m.new_device_state()
    resyncs = compressions = 0
    try:
        for step, chunk, rng in random_stream(seed, 40):
            T = host.spkcache_len + host.fifo_len + chunk.shape[0]
            preds = rng.random((T, 4)).astype(np.float32) ** (3.0 if silence else 1.0)
            if silence:
                preds[rng.random(T) < 0.3] *= 0.02
            lc, rc = (0 if step == 0 else 1), 1
            n_before = len(rec.gaps)
            out_h = sf.streaming_update(sp, host, chunk, preds, lc, rc)
            out_d = dev.update(chunk, preds, lc, rc)
            compressions += len(rec.gaps) - n_before
            assert out_h.shape == out_d.shape and beq(out_h, out_d), step
            dstate, _ = dev.to_host()
            if assert_state_rule1(host, dstate, n_before, rec):
                resyncs += 1
                dev.load(host)
        assert resyncs <= 2, resyncs
        assert compressions >= 2
        if silence:
            assert host.n_sil_frames > 0
    finally:
        dev.close()


def full_state(sp, rng, d=512, n_spk=4, preds_fn=None):
    """A state with a full cache and a full FIFO (the next step pops and compresses)."""
    st = sf.SortformerState(rng.standard_normal((sp.spkcache_len, d)).astype(np.float32),
                            rng.random((sp.spkcache_len, n_spk)).astype(np.float32),
                            rng.standard_normal((sp.fifo_len, d)).astype(np.float32),
                            rng.random((sp.fifo_len, n_spk)).astype(np.float32),
                            (0.1 * rng.standard_normal(d)).astype(np.float32), sp.spkcache_len, sp.fifo_len, 7)
    return st


def edge_preds(kind, T, rng):
    if kind == "duplicated":
        row = np.array([0.9, 0.7, 0.6, 0.8], np.float32)
        p = np.tile(row, (T, 1))
        p[::3] = np.array([0.95, 0.55, 0.65, 0.75], np.float32)
        return p
    if kind == "all_silent":
        return np.full((T, 4), 0.01, np.float32)
    if kind == "one_speaker":
        p = np.full((T, 4), 0.05, np.float32)
        p[:, 0] = (0.6 + 0.39 * rng.random(T)).astype(np.float32)
        return p
    if kind == "few_finite":
        p = np.full((T, 4), 0.1, np.float32)
        hot = rng.choice(T, size=5, replace=False)
        p[hot, hot % 4] = 0.9
        return p
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["duplicated", "all_silent", "one_speaker", "few_finite"])
def test_compression_edge_cases_bitwise(small, kind):
    m, sp = small, small.cache
    rng = np.random.default_rng(["duplicated", "all_silent", "one_speaker", "few_finite"].index(kind))
    host = full_state(sp, rng)
    if kind == "duplicated":          # identical cache rows: exact score ties resolve to the lowest index
        host.spkcache[1::2] = host.spkcache[0::2]
    dev = m.new_device_state()
    try:
        dev.load(host)
        chunk = rng.standard_normal((25, 512)).astype(np.float32)
        preds = edge_preds(kind, host.spkcache_len + host.fifo_len + 25, rng)
        host.spkcache_preds[:] = preds[: sp.spkcache_len]
        dev.load(host)
        out_h = sf.streaming_update(sp, host, chunk, preds, 1, 1)
        out_d = dev.update(chunk, preds, 1, 1)
        st, _ = dev.to_host()
        assert beq(out_h, out_d)
        assert (host.spkcache_len, host.fifo_len, host.n_sil_frames) == (st.spkcache_len, st.fifo_len, st.n_sil_frames)
        for name in ("spkcache", "spkcache_preds", "fifo", "fifo_preds", "mean_sil_emb"):
            assert beq(getattr(host, name), getattr(st, name)), name
        if kind == "all_silent":
            assert np.array_equal(st.spkcache, np.tile(st.mean_sil_emb, (sp.spkcache_len, 1))) and not st.spkcache_preds.any()
    finally:
        dev.close()


def test_full_depth_session_teacher_forced(full, monkeypatch):
    """20 chunks of speech through HipSortformerDiarizationOnline, host state and device state on one model; before each
    chunk the host's state and kept rows are loaded into the device session."""
    m = full
    rec = CompressRecorder(monkeypatch)
    host = HipSortformerDiarizationOnline(m)
    dev = HipSortformerDiarizationOnline(m)
    dev.streaming_state = m.new_device_state()
    audio = speech_like(20.0, seed=7).astype(np.float32)
    overflowed = False
    n_comp = 0
    try:
        for k in range(20):
            prev = host._previous_chunk_features[-99:] if host._previous_chunk_features is not None else None
            dev.streaming_state.load(host.streaming_state, prev)
            for o in (host, dev):
                o.insert_audio_chunk(audio[k * 16000:(k + 1) * 16000])
            n_before = len(rec.gaps)
            sh, sd = host.diarize_sync(), dev.diarize_sync()
            n_comp += len(rec.gaps) - n_before
            assert [(s.speaker, s.start, s.end) for s in sh] == [(s.speaker, s.start, s.end) for s in sd], k
            assert beq(host.total_preds, dev.total_preds), k
            assert dev._previous_chunk_features is None
            st, kept = dev.streaming_state.to_host()
            assert beq(kept, host._previous_chunk_features[-99:]), k
            assert_state_rule1(host.streaming_state, st, n_before, rec)
            overflowed |= host.streaming_state.spkcache_len > 0
        assert overflowed and n_comp >= 1
    finally:
        dev.close()


def test_free_running_session_equals_host_path_up_to_a_near_tie(full, monkeypatch):
    m = full
    rec = CompressRecorder(monkeypatch)
    host = HipSortformerDiarizationOnline(m)
    dev = HipSortformerDiarizationOnline(m)
    dev.streaming_state = m.new_device_state()
    audio = speech_like(20.0, seed=9).astype(np.float32)
    tied = False
    try:
        for k in range(20):
            for o in (host, dev):
                o.insert_audio_chunk(audio[k * 16000:(k + 1) * 16000])
            n_before = len(rec.gaps)
            sh, sd = host.diarize_sync(), dev.diarize_sync()
            if tied:
                break
            assert [(s.speaker, s.start, s.end) for s in sh] == [(s.speaker, s.start, s.end) for s in sd], k
            assert beq(host.total_preds, dev.total_preds), k
            tied = any(g < NEAR for g in rec.gaps[n_before:])
        assert dev.streaming_state.spkcache_len == host.streaming_state.spkcache_len
    finally:
        dev.close()


def test_device_and_host_sessions_stack_and_stay_bitwise(full):
    """Four device sessions and four host sessions released together through a barrier: every result (activities, kept
    rows, state) bit for bit its step alone, and the eight steps shared stacked chains."""
    m = full
    sessions = []
    for t in range(8):
        a = speech_like(4.0, seed=40 + t).astype(np.float32)
        on_dev = t % 2 == 0
        st = m.new_device_state() if on_dev else m.new_state()
        prev = None
        for k in range(3):      # some history first, different per session
            pcm = a[k * 16000:(k + 1) * 16000]
            if on_dev:
                m.forward_streaming_step_session_pcm(pcm, st, 8 if k else 0, 8)
            else:
                _, feats = m.forward_streaming_step_pcm(pcm, prev, st, 8 if k else 0, 8)
                prev = feats[-99:]
        sessions.append(dict(dev=on_dev, st=st, prev=prev, pcm=a[48000:64000]))

    def snapshot(s):
        return s["st"].to_host() if s["dev"] else (copy.deepcopy(s["st"]), None if s["prev"] is None else s["prev"].copy())

    def restore(s, snap):
        if s["dev"]:
            s["st"].load(*snap)
        else:
            s["st"] = copy.deepcopy(snap[0])

    def step(s):
        if s["dev"]:
            return m.forward_streaming_step_session_pcm(s["pcm"], s["st"], 8, 8), None
        return m.forward_streaming_step_pcm(s["pcm"], s["prev"], s["st"], 8, 8)

    def outcome(s, r):
        st, kept = s["st"].to_host() if s["dev"] else (s["st"], r[1][-99:])
        return r[0], kept, st

    try:
        snaps = [snapshot(s) for s in sessions]
        alone = [outcome(s, step(s)) for s in sessions]
        for s, snap in zip(sessions, snaps):
            restore(s, snap)
        before = m.stats()
        gate = threading.Barrier(8)
        got = [None] * 8

        def worker(i):
            gate.wait()
            got[i] = outcome(sessions[i], step(sessions[i]))
        th = [threading.Thread(target=worker, args=(i,)) for i in range(8)]
        [t.start() for t in th]
        [t.join() for t in th]
        after = m.stats()
        assert after["session_steps"] - before["session_steps"] == 8
        assert after["stacked_steps"] - before["stacked_steps"] < 8, (before, after)
        for (pa, ka, sa), (pg, kg, sg) in zip(alone, got):
            assert beq(pa, pg) and beq(ka, kg)
            assert (sa.spkcache_len, sa.fifo_len, sa.n_sil_frames) == (sg.spkcache_len, sg.fifo_len, sg.n_sil_frames)
            for name in ("spkcache", "spkcache_preds", "fifo", "fifo_preds", "mean_sil_emb"):
                assert beq(getattr(sa, name), getattr(sg, name)), name
    finally:
        for s in sessions:
            if s["dev"]:
                s["st"].close()


def test_session_contract(small):
    m = small
    st = m.new_device_state()
    try:
        # the model refuses to go while a session lives, and frees nothing
        assert m.lib.wlk_sf_destroy(m._h) == -3
        chunk = np.random.default_rng(0).standard_normal((13, 512)).astype(np.float32)
        out = st.update(chunk, np.full((13, 4), 0.7, np.float32), 0, 1)
        assert out.shape == (12, 4) and st.fifo_len == 12
        pcm = speech_like(1.0, seed=1).astype(np.float32)
        m.forward_streaming_step_session_pcm(pcm, st, 0, 8)
        # a session of another model
        other = sf.HipSortformerModel(m.dims, sf.synth_sortformer_state_dict(m.dims, 22))
        try:
            foreign = other.new_device_state()
            with pytest.raises(_lib.WlkError):
                m.forward_streaming_step_session_pcm(pcm, foreign, 8, 8)
            with pytest.raises(_lib.WlkError):
                m.forward_streaming_step(np.zeros((200, 128), np.float32), foreign, 8, 8)
        finally:
            other.close()                 # closes `foreign` first
        assert not foreign._h
        # an audio chunk longer than the step's buffer; an extractor of another geometry; activity rows that do not fit
        with pytest.raises(_lib.WlkError):
            m.forward_streaming_step_session_pcm(np.zeros(64001, np.float32), st, 8, 8)
        mel80 = HipMelSpectrogram(n_mels=80)
        try:
            with pytest.raises(_lib.WlkError):
                m.forward_streaming_step_session_pcm(pcm, st, 8, 8, mel=mel80)
        finally:
            mel80.close()
        with pytest.raises(_lib.WlkError):
            st.update(chunk, np.zeros((5, 4), np.float32), 1, 1)
        assert st.fifo_len == 24                                # the failed calls left the state as it was
        m.forward_streaming_step_session_pcm(pcm, st, 8, 8)
    finally:
        st.close()
    # model.close() closes the states it still tracks
    third = sf.HipSortformerModel(m.dims, sf.synth_sortformer_state_dict(m.dims, 23), device_state=True)
    a, b = third.new_state(), third.new_device_state()
    assert isinstance(a, sf.DeviceSortformerState)
    third.close()
    assert not a._h and not b._h and not third._h
