"""The three audio front ends on the GPU through their production entry points - wlk_encode + export("mel") (streaming
log-mel), wlk_log_mel (whole file), wlk_melspec_run, wlk_vad_stream_run / _run_pcm16 / wlk_vad_group_run - each output judged
per element against the float64 reference of tests/frontend_reference.py on the cases of tests/frontend_cases.py.

Tolerance (tests/select_reference.py: value_tolerance, unchanged): a value may be off by 4 x the error the float32
restatement has on the same case (floor 2^-22 * max(1, |reference|)), times frontend_reference.FAMILY_FACTOR (1 unless a
family needed more on an MI355X).  No element is left out.  Beside the values: the frame count and content_mel_len, the
frames past the audio (one value, the floor), a second launch (the same bits), the refusal of a signal the reflection does
not fit (nothing touched), buffers behind guard words.  Every case writes its worst error, the allowed error and their
ratio to frontend_report.json in the directory WLK_REPORT_DIR names (default: test_reports/)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import frontend_cases as FC
import frontend_reference as FR
from whisperlivekit_amd import _lib, synth
from whisperlivekit_amd import vad as V
from whisperlivekit_amd.dims import ModelDims
from whisperlivekit_amd.engine import HipWhisperModel, hann_window_periodic, pack_state_dict

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {"cases": {}, "worst_of_allowed": {}, "family_factor": dict(FR.FAMILY_FACTOR), "kernel_factor": FR.KERNEL_FACTOR}
WLK_ERR_ARG = -1
GUARD = np.uint32(0x7FC12345)           # a NaN with a payload


def guard(shape):
    return np.full(shape, GUARD, np.uint32).view(np.float32)


def is_guard(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint32) == GUARD))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def judge(family, name, outputs):
    """outputs = {tag: (got, ref, f32)} -> failures; the entries go to the report"""
    failures, rep = [], {}
    for tag, (got, ref, f32) in outputs.items():
        entry, fail = FR.judge(tag, got, ref, f32, family)
        rep[tag] = entry
        print(family, name, tag, json.dumps(entry))
        if fail:
            failures.append(f"{name}: {fail}")
        worst = REPORT["worst_of_allowed"].setdefault(family, dict(of_allowed=0.0, case=None))
        if entry["of_allowed"] > worst["of_allowed"]:
            worst.update(of_allowed=entry["of_allowed"], case=f"{name}/{tag}")
    REPORT["cases"][f"{family}/{name}"] = rep
    out = os.environ.get("WLK_REPORT_DIR") or os.path.join(ROOT, "test_reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "frontend_report.json"), "w") as fh:
        json.dump(REPORT, fh, indent=1, sort_keys=True)
    return failures


# ----------------------------------------------------------------------------------------------------------------------
# Whisper log-mel: micro-width models of 80 and 128 bins, each with the slaney and the `edges` bank
# ----------------------------------------------------------------------------------------------------------------------
_models = {}


def mel_model(bank_kind, n_mels):
    key = (bank_kind, n_mels)
    if key not in _models:
        dims = ModelDims(n_mels, 1500, 128, 2, 1, 51866 if n_mels == 128 else 51864, 448, 128, 2, 1)
        m = HipWhisperModel(dims)
        m.upload_packed({**pack_state_dict(dims, synth.synth_state_dict(dims, 5)),
                         "mel.filters": np.ascontiguousarray(FC.bank(bank_kind, n_mels))})
        m.set_alignment_heads([(0, 0)])
        m.finalize()
        _models[key] = m
    return _models[key]


@pytest.fixture(scope="module", autouse=True)
def close_models():
    yield
    for m in _models.values():
        m.close()
    _models.clear()


def log_mel_refs(c):
    args = (c["audio"], c["bank"], c["padding"])
    w = hann_window_periodic()                        # the window pack_state_dict gives the model
    return FR.log_mel(*args, dt=np.float64, window=w), FR.log_mel(*args, dt=np.float32, window=w), \
        FR.log_mel_parts(*args, window=w)[2]


def check_past_audio(got, past, gmax64, failures):
    """frames that only see padding are exactly (max(-10, gmax - 8) + 4) / 4: one value - (-10 + 4) / 4 where the
    reference's max - 8 is clearly under -10, the smallest value of the whole output (every floored element has its bits)
    where it is clearly above; its distance from the reference is judged with the rest.  (A frame the kernel computes from
    zeros may sit one ulp under the fill: the device's log10f(1e-10f) is -10.000001, see DESIGN.md.)"""
    if past >= got.shape[1]:
        return
    tail = got[:, past:]
    if np.unique(bits(tail)).size != 1:
        failures.append(f"{np.unique(bits(tail)).size} different values in the frames past the audio")
    elif gmax64 - 8.0 < -10.0 - 1e-3 and tail[0, 0] != np.float32(-1.5):
        failures.append(f"the frames past the audio hold {tail[0, 0]!r}, not (-10 + 4) / 4")
    elif gmax64 - 8.0 > -10.0 + 1e-3 and tail[0, 0] != got.min():
        failures.append(f"the frames past the audio hold {tail[0, 0]!r}, the output's floor is {got.min()!r}")


@pytest.mark.parametrize("name", FC.LOG_MEL_NAMES)
def test_log_mel_whole_file(name):
    c = FC.log_mel_case(name)
    ref, f32, gmax = log_mel_refs(c)
    sess = mel_model(c["bank_kind"], c["n_mels"]).new_session(batched=False)
    try:
        got = sess.log_mel(c["audio"], c["padding"])
        again = sess.log_mel(c["audio"], c["padding"])
    finally:
        sess.close()
    assert got.shape == ref.shape == (c["n_mels"], (c["audio"].size + c["padding"]) // 160)
    failures = judge("log_mel", name, {"wlk_log_mel": (got, ref, f32)})
    if not np.array_equal(bits(got), bits(again)):
        failures.append(f"a second call differs in {int((bits(got) != bits(again)).sum())} elements")
    check_past_audio(got, FR.log_mel_past_audio(c["audio"].size, c["padding"]), gmax, failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("n, padding", FC.LOG_MEL_REFUSED)
def test_log_mel_refuses_what_the_reflection_does_not_fit(n, padding):
    """n + padding <= 200: WLK_ERR_ARG, and neither the output nor the frame count is touched"""
    sess = mel_model("slaney", 80).new_session(batched=False)
    lib = _lib.load()
    pcm = np.ascontiguousarray(FC.signal("noise", max(n, 1)))
    out = guard(80 * 8)
    frames = C.c_int32(-7)
    try:
        for mel in (None, out.ctypes.data_as(C.POINTER(C.c_float))):
            rc = lib.wlk_log_mel(sess._h, pcm.ctypes.data_as(C.POINTER(C.c_float)), n, padding, mel, out.size, C.byref(frames))
            assert rc == WLK_ERR_ARG and frames.value == -7 and is_guard(out), (rc, frames.value)
        # the session is as it was: the smallest signal it accepts goes through
        one = sess.log_mel(FC.signal("noise", 201), 0)
        assert one.shape == (80, 1) and np.all(np.isfinite(one))
    finally:
        sess.close()


def run_script(sess, script):
    """-> (content_mel_len, mel [n_mels][3000]) of the last encode"""
    cml = None
    for step in script:
        if step[0] == "append":
            sess.append(FC.signal(step[1])[step[2]:step[3]])
        elif step[0] == "pcm16":
            sess.append_pcm16(FC.to_pcm16(FC.signal(step[1])[step[2]:step[3]]))
        elif step[0] == "drop":
            sess.drop_front(step[1])
        else:
            cml = sess.encode()
    return cml, sess.export("mel").reshape(sess.model.dims.n_mels, 3000).copy()


@pytest.mark.parametrize("name", FC.STREAM_NAMES)
def test_log_mel_streaming(name):
    c = FC.stream_case(name)
    full, full32, gmax = log_mel_refs(c)
    ref, f32 = full[:, :3000], full32[:, :3000]
    want_cml = (full.shape[1] - 3000) // 2
    model = mel_model(c["bank_kind"], c["n_mels"])
    sess, fresh = model.new_session(batched=False), model.new_session(batched=False)
    try:
        cml, got = run_script(sess, c["script"])
        assert sess.audio_len == c["audio"].size
        cml2 = sess.encode()                                      # nothing new: every frame comes from the session's cache
        again = sess.export("mel").reshape(c["n_mels"], 3000).copy()
        fresh.append(c["audio"])                                  # the same buffer in one piece, nothing cached
        cml3 = fresh.encode()
        whole = fresh.export("mel").reshape(c["n_mels"], 3000).copy()
    finally:
        sess.close()
        fresh.close()
    failures = judge("log_mel", "stream_" + name, {"wlk_encode": (got, ref, f32)})
    if not (cml == cml2 == cml3 == want_cml):
        failures.append(f"content_mel_len {cml}, {cml2}, {cml3}: the reference gives {want_cml}")
    if not np.array_equal(bits(got), bits(again)):
        failures.append(f"a second encode differs in {int((bits(got) != bits(again)).sum())} elements")
    if not np.array_equal(bits(got), bits(whole)):
        failures.append(f"the buffer appended in one piece differs in {int((bits(got) != bits(whole)).sum())} elements")
    check_past_audio(got, FR.log_mel_past_audio(c["audio"].size, c["padding"]), gmax, failures)
    assert not failures, "\n".join(failures)


# ----------------------------------------------------------------------------------------------------------------------
# mel-spectrogram
# ----------------------------------------------------------------------------------------------------------------------
def run_melspec(c):
    """-> (frames, out [frames][n_mels], the same from a second run)"""
    lib = _lib.load()
    h = C.c_void_p()
    filters, window = np.ascontiguousarray(c["bank"]), np.ascontiguousarray(c["window"])
    audio = np.ascontiguousarray(c["audio"])
    _lib.check(lib.wlk_melspec_create(0, c["n_fft"], c["win_length"], c["hop"], c["n_mels"], filters.ctypes.data_as(C.c_void_p),
                                      window.ctypes.data_as(C.c_void_p), c["preemph"], c["guard"], max(audio.size, c["n_fft"]),
                                      C.byref(h)))
    try:
        outs = []
        cap = audio.size // c["hop"] + 1
        for _ in range(2):
            out = guard((cap + 1, c["n_mels"]))
            n = C.c_int(-7)
            _lib.check(lib.wlk_melspec_run(h, audio.ctypes.data_as(C.c_void_p), audio.size, out.ctypes.data_as(C.c_void_p), cap,
                                           C.byref(n)))
            assert n.value == cap, (n.value, cap)
            assert is_guard(out[cap:]), "wrote behind its frames"
            outs.append(out[:cap].copy())
        return cap, outs[0], outs[1]
    finally:
        lib.wlk_melspec_destroy(h)


@pytest.mark.parametrize("name", FC.MELSPEC_NAMES)
def test_melspec(name):
    c = FC.melspec_case(name)
    args = FC.melspec_args(c)
    ref, f32 = FR.melspec(*args, dt=np.float64, window=c["window"]), FR.melspec(*args, dt=np.float32, window=c["window"])
    frames, got, again = run_melspec(c)
    assert frames == c["audio"].size // c["hop"] + 1 and got.shape == ref.shape
    failures = judge("melspec", name, {"wlk_melspec_run": (got, ref, f32)})
    if not np.array_equal(bits(got), bits(again)):
        failures.append(f"a second run differs in {int((bits(got) != bits(again)).sum())} elements")
    assert not failures, "\n".join(failures)


# ----------------------------------------------------------------------------------------------------------------------
# Silero VAD
# ----------------------------------------------------------------------------------------------------------------------
def vad_refs(sd, audio, state_after):
    return (FR.vad_stream(sd, audio, np.float64, state_after=state_after),
            FR.vad_stream(sd, audio, np.float32, state_after=state_after))


def run_in_calls(model, audio, calls, pcm16=False):
    """-> (probs, {windows done: (h, c)} after every call)"""
    probs, states, at = [], {}, 0
    for n in calls:
        chunk = audio[512 * at:512 * (at + n)]
        probs.append(model.probs_pcm16(chunk) if pcm16 else model.probs(chunk))
        at += n
        states[at] = model.state()
    return np.concatenate(probs), states


@pytest.mark.parametrize("name", FC.VAD_NAMES)
def test_vad(name):
    c = FC.vad_case(name)
    sd, audio, W = c["sd"], np.ascontiguousarray(c["audio"]), c["n_windows"]
    ref, f32 = vad_refs(sd, audio, c["state_after"])
    weights = V.HipSileroVADWeights(dict(sd))
    a, b, other = (V.HipSileroVAD(weights, max_windows=64) for _ in range(3))
    group = V.HipSileroVADGroup(weights, max_streams=4, max_windows=64)
    outputs, failures = {}, []
    try:
        # calls of 1, 1 and the rest: the state after 1, 2 and all windows (the forget gate shows from window 2 on)
        probs, states = run_in_calls(a, audio, [1, 1, W - 2])
        outputs["probs"] = (probs, ref["probs"], f32["probs"])
        for n in c["state_after"]:
            for k, key in enumerate("hc"):
                outputs[f"{key}_after_{n}"] = (states[n][k], ref["states"][n][k], f32["states"][n][k])
        # calls of 1, 7 and the rest on a fresh stream: the context carries between calls
        probs_b, states_b = run_in_calls(b, audio, c["calls"])
        outputs["probs_calls_1_7_rest"] = (probs_b, ref["probs"], f32["probs"])
        outputs["h_calls_1_7_rest"] = (states_b[W][0], ref["h"], f32["h"])
        outputs["c_calls_1_7_rest"] = (states_b[W][1], ref["c"], f32["c"])
        # after reset_states: the first stream again, in one call
        a.reset_states()
        probs_r, states_r = run_in_calls(a, audio, [W])
        outputs["probs_after_reset"] = (probs_r, ref["probs"], f32["probs"])
        outputs["c_after_reset"] = (states_r[W][1], ref["c"], f32["c"])
        # a group call beside a second stream (fewer windows, other audio), cut in two so that both contexts carry
        audio2 = np.ascontiguousarray(audio.reshape(W, 512)[::-1][:20].reshape(-1))
        ref2, f322 = vad_refs(sd, audio2, (20,))
        b.reset_states()
        g1 = group.probs([b, other], [audio[:512 * 5], audio2[:512 * 9]])
        g2 = group.probs([other, b], [audio2[512 * 9:], audio[512 * 5:]])
        outputs["probs_group"] = (np.concatenate([g1[0], g2[1]]), ref["probs"], f32["probs"])
        outputs["probs_group_other"] = (np.concatenate([g1[1], g2[0]]), ref2["probs"], f322["probs"])
        outputs["h_group"] = (b.state()[0], ref["h"], f32["h"])
        outputs["c_group_other"] = (other.state()[1], ref2["c"], f322["c"])
        # once from int16
        pcm = FC.to_pcm16(audio)
        ref16, f3216 = vad_refs(sd, pcm.astype(np.float32) / np.float32(32768.0), (W,))
        a.reset_states()
        probs16, states16 = run_in_calls(a, pcm, c["calls"], pcm16=True)
        outputs["probs_pcm16"] = (probs16, ref16["probs"], f3216["probs"])
        outputs["h_pcm16"] = (states16[W][0], ref16["h"], f3216["h"])
        other.reset_states()
        g16 = group.probs([other], [pcm])
        if not np.array_equal(bits(g16[0]), bits(probs16)):
            failures.append("int16 through the group call differs from int16 through the stream call")
        # however the windows are cut into calls, the bits are the same
        for tag, p in (("calls of 1, 7, rest", probs_b), ("one call after reset", probs_r), ("the group call", outputs["probs_group"][0])):
            if not np.array_equal(bits(p), bits(probs)):
                failures.append(f"{tag}: {int((bits(p) != bits(probs)).sum())} probabilities differ from calls of 1, 1, rest")
    finally:
        group.close()
        for m in (a, b, other):
            m.close()
        weights.close()
    failures += judge("vad", name, outputs)
    assert not failures, "\n".join(failures)
