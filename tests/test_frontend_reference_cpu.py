"""The references of tests/frontend_reference.py against independent statements, on every case of tests/frontend_cases.py,
without a GPU: the float64 log-mel against oracle/whisper_oracle.log_mel_spectrogram, the float64 mel-spectrogram against
oracle/sortformer_oracle.nemo_log_mel (both run in double on the same float32 inputs: their float32 FFT is itself a
restatement, further from float64 than the kernels' stated arithmetic), the float64 VAD against oracle/vad_oracle in double,
for the real and the random weights; the float32 restatement against the tolerance it defines; every deliberate mistake
of the reference module against that tolerance - exactly the allowed error tests/test_gpu_frontend.py uses, family factor
included - on every case it applies to (frontend_cases.*_mutants say which cases cannot see a mistake, and why); and the
conditions the cases were built for."""
import functools

import numpy as np
import pytest
import torch

import frontend_cases as FC
import frontend_reference as FR
from oracle import vad_oracle, whisper_oracle
from oracle.sortformer_oracle import nemo_log_mel
from whisperlivekit_amd.engine import hann_window_periodic


def caught(mutated, ref, allowed):
    """the mistake shows: somewhere it is further from the reference than a kernel may be"""
    err = FR.abs_err(mutated, ref)
    return bool((err > allowed).any()), float((err / allowed).max())


def restatement_passes(ref, f32, family):
    assert ref.dtype == np.float64 and f32.dtype == np.float32 and ref.shape == f32.shape
    entry, fail = FR.judge("restatement", f32, ref, f32, family)
    assert fail is None and np.isfinite(entry["restatement_err"]), (entry, fail)


# ----------------------------------------------------------------------------------------------------------------------
# log-mel
# ----------------------------------------------------------------------------------------------------------------------
def any_log_mel_case(name):
    return FC.stream_case(name) if name in FC.STREAM else FC.log_mel_case(name)


@functools.lru_cache(maxsize=None)
def log_mel_refs(name):
    c = any_log_mel_case(name)
    w = hann_window_periodic()                                # the window the model is given
    args = (c["audio"], c["bank"], c["padding"])
    ref, f32 = FR.log_mel(*args, dt=np.float64, window=w), FR.log_mel(*args, dt=np.float32, window=w)
    return c, args, w, ref, f32, FR.allowed_error(ref, f32, "log_mel")


def test_the_window_of_the_reference_is_the_window_of_the_model():
    """torch computes its window in float32 and lands a few ulps from the rounded exact one: the window is an INPUT of the
    kernel, so the references take the model's"""
    a, b = FR.hann(400, periodic=True), hann_window_periodic()
    assert a.dtype == b.dtype == np.float32 and np.abs(a.astype(np.float64) - b).max() <= 2.0 ** -21
    assert FR.hann(400, periodic=False)[-1] == 0.0 and FR.hann(400, periodic=True)[-1] != 0.0


@pytest.mark.parametrize("name", FC.LOG_MEL_NAMES + FC.STREAM_NAMES)
def test_log_mel_reference_and_mutants(name):
    c, args, w, ref, f32, allowed = log_mel_refs(name)
    n, padding = c["audio"].size, c["padding"]
    assert ref.shape == (c["n_mels"], FR.log_mel_frames(n, padding)) and np.all(np.isfinite(ref))
    restatement_passes(ref, f32, "log_mel")
    # the oracle in double on the same float32 samples, window and bank
    want = whisper_oracle.log_mel_spectrogram(torch.from_numpy(np.array(c["audio"])).double(),
                                              torch.from_numpy(np.array(c["bank"])), padding).numpy()
    assert want.dtype == np.float64 and want.shape == ref.shape
    assert (FR.abs_err(want, ref) <= allowed).all(), float((FR.abs_err(want, ref) / allowed).max())
    # ... and as the other tests use it, in float32, under the tolerance they give the kernel
    want32 = whisper_oracle.log_mel_spectrogram(torch.from_numpy(np.array(c["audio"])), torch.from_numpy(np.array(c["bank"])),
                                                padding).numpy()
    assert want32.dtype == np.float32 and FR.abs_err(want32, ref).max() <= 1e-4
    # frames past the audio are one value
    parts = FR.log_mel_parts(*args, window=w)
    past = FR.log_mel_past_audio(n, padding)
    tail = (max(-10.0, parts[2] - 8.0) + 4.0) / 4.0
    assert past == ref.shape[1] or np.all(ref[:, past:] == tail)
    mutants = FC.log_mel_mutants(c, parts)
    assert set(mutants) <= set(FR.LOG_MEL_MUTANTS) and mutants
    for m in mutants:
        hit, ratio = caught(FR.log_mel(*args, window=w, mutant=m), ref, allowed)
        assert hit, f"{name} cannot tell '{m}' from the reference (largest error {ratio:.3g} of the allowed)"
    if c["streaming"]:
        got, cml = FR.log_mel_streaming(c["audio"], c["bank"], window=w)
        assert np.array_equal(got, ref[:, :3000]) and cml == (n + 480000) // 160 // 2 - 1500 and got.shape[1] == 3000


def test_every_log_mel_mutant_meets_cases_and_the_cases_hit_what_they_were_written_for():
    seen = {m: 0 for m in FR.LOG_MEL_MUTANTS}
    for name in FC.LOG_MEL_NAMES + FC.STREAM_NAMES:
        c = any_log_mel_case(name)
        for m in FC.log_mel_mutants(c, FR.log_mel_parts(c["audio"], c["bank"], c["padding"])):
            seen[m] += 1
    assert all(v >= 2 for v in seen.values()), seen
    cases = [FC.LOG_MEL[n] for n in FC.LOG_MEL_NAMES]
    totals = {FR.log_mel_frames(n, p) for _, n, p, _, _ in cases}
    assert any(t % 64 == 0 for t in totals) and any(t % 64 for t in totals) and 1 in totals
    assert {0, 1, 100, 199, 200, 480000} <= {p for _, _, p, _, _ in cases}
    assert 201 in {n + p for _, n, p, _, _ in cases} and all(n + p <= 200 for n, p in FC.LOG_MEL_REFUSED)
    assert {(b, m) for _, _, _, b, m in cases} == {(b, m) for b in ("slaney", "edges") for m in (80, 128)}
    assert {s for s, *_ in cases} >= {"speech", "noise", "dc_tone", "impulse", "square", "bursts", "quiet"}
    # the right reflection: all of its 40 samples real, one real, none
    assert FC.right_reflection_reach(16000, 0) == (40, 40) and FC.right_reflection_reach(4120, 40) == (40, 1)
    assert FC.right_reflection_reach(4119, 41) == (40, 0) and FC.right_reflection_reach(201, 0)[0] == 0
    for kind in ("speech", "noise", "dc_tone", "impulse", "square", "bursts", "quiet"):
        assert 0.2 * 16000 <= FC.signal(kind).size <= 1.5 * 16000
    drop = FC.stream_case("drop_front_speech_edges128")
    assert drop["audio"][0] != 0.0 and drop["audio"].size == 19000 - 3200
    assert any(s[0] == "pcm16" for s in FC.STREAM["pcm16_bursts_slaney128"][2])


@pytest.mark.parametrize("n_mels", [80, 128])
def test_the_edges_bank_has_the_rows_it_names(n_mels):
    b, s = FC.bank("edges", n_mels), FC.bank("slaney", n_mels)
    R = FC.EDGE_ROWS
    assert np.flatnonzero(b[R["bin0"]]).tolist() == [0] and np.flatnonzero(b[R["nyquist"]]).tolist() == [200]
    assert np.flatnonzero(b[R["low4"]]).tolist() == [0, 1, 2, 3] and np.all(b[R["all_bins"]] > 0) and not b[R["empty"]].any()
    hole = np.flatnonzero(b[R["hole"]])
    assert hole[0] == 50 and hole[-1] == 60 and hole.size == 9
    assert np.array_equal(b[6:], s[6:]) and (b >= 0).all()
    assert not s[:, 0].any() and not s[:, 200].any()         # what the production bank never reaches
    assert max(np.count_nonzero(r) for r in s) <= 14


def test_the_quiet_signal_shows_the_clamp():
    """between 5 % and 95 % of its float64 energies lie under 1e-10 and its largest L is under -2: the floor max - 8 is
    below -10"""
    for n_mels in (80, 128):
        for kind in ("slaney", "edges"):
            mel, L, gmax = FR.log_mel_parts(FC.signal("quiet"), FC.bank(kind, n_mels), 0)
            live = mel[[i for i in range(n_mels) if FC.bank(kind, n_mels)[i].any()]]
            frac = float((live < 1e-10).mean())
            assert 0.05 <= frac <= 0.95 and gmax < -2.0, (n_mels, kind, frac, gmax)


# ----------------------------------------------------------------------------------------------------------------------
# mel-spectrogram
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FC.MELSPEC_NAMES)
def test_melspec_reference_and_mutants(name):
    c = FC.melspec_case(name)
    args = FC.melspec_args(c)
    ref, f32 = FR.melspec(*args, dt=np.float64, window=c["window"]), FR.melspec(*args, dt=np.float32, window=c["window"])
    assert ref.shape == (c["audio"].size // c["hop"] + 1, c["n_mels"]) and np.all(np.isfinite(ref))
    restatement_passes(ref, f32, "melspec")
    allowed = FR.allowed_error(ref, f32, "melspec")
    # the oracle in double, with torch's float32 window as the reference's window
    tw = torch.hann_window(c["win_length"], periodic=False).numpy()
    assert np.abs(tw.astype(np.float64) - c["window"]).max() <= 2.0 ** -21
    want = nemo_log_mel(c["audio"], c["bank"], c["n_fft"], c["win_length"], c["hop"], c["preemph"], c["guard"],
                        seq_len_plus_one=True, double=True)
    mine = FR.melspec(*args, dt=np.float64, window=tw)
    assert want.dtype == np.float64 and want.shape == ref.shape
    assert (FR.abs_err(want, mine) <= allowed).all(), float((FR.abs_err(want, mine) / allowed).max())
    want32 = nemo_log_mel(c["audio"], c["bank"], c["n_fft"], c["win_length"], c["hop"], c["preemph"], c["guard"],
                          seq_len_plus_one=True)
    assert want32.dtype == np.float32 and FR.abs_err(want32, mine).max() <= 1e-3
    mutants = FC.melspec_mutants(c)
    assert set(mutants) <= set(FR.MELSPEC_MUTANTS)
    for m in mutants:
        hit, ratio = caught(FR.melspec(*args, dt=np.float64, window=c["window"], mutant=m), ref, allowed)
        assert hit, f"{name} cannot tell '{m}' from the reference (largest error {ratio:.3g} of the allowed)"


def test_every_melspec_mutant_meets_cases_and_the_settings_are_there():
    seen = {m: 0 for m in FR.MELSPEC_MUTANTS}
    for name in FC.MELSPEC_NAMES:
        for m in FC.melspec_mutants(FC.melspec_case(name)):
            seen[m] += 1
    assert all(v >= 2 for v in seen.values()), seen
    S = list(FC.MELSPEC.values())
    assert (512, 400, 160, 128, 0.97, FC.NEMO_GUARD) in {s[:6] for s in S} and (256, 200, 80, 40) in {s[:4] for s in S}
    assert any(s[0] == s[1] for s in S) and any((s[0] - s[1]) % 2 for s in S) and any(s[3] == 256 for s in S)
    assert any(s[4] == 0.0 for s in S) and any(s[8] < s[0] // 2 for s in S)
    for n_fft, n_mels in ((512, 128), (256, 40), (400, 80), (512, 256), (512, 64)):
        b = FC.bank("edges", n_mels, n_fft)
        assert b.shape == (n_mels, n_fft // 2 + 1) and b[0, 0] > 0 and b[1, n_fft // 2] > 0


# ----------------------------------------------------------------------------------------------------------------------
# VAD
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def vad_refs(name):
    c = FC.vad_case(name)
    ref = FR.vad_stream(c["sd"], c["audio"], np.float64, state_after=c["state_after"])
    f32 = FR.vad_stream(c["sd"], c["audio"], np.float32, state_after=c["state_after"])
    return c, ref, f32


def vad_outputs(run, state_after):
    """the outputs the GPU test judges: the probabilities, and (h, c) after 1, 2 and all windows"""
    out = {"probs": run["probs"]}
    for n in state_after:
        out[f"h_after_{n}"], out[f"c_after_{n}"] = run["states"][n]
    return out


@pytest.mark.parametrize("name", FC.VAD_NAMES)
def test_vad_reference_and_mutants(name):
    c, ref, f32 = vad_refs(name)
    W = c["n_windows"]
    assert W == 33 and sum(c["calls"]) == W and c["calls"][:2] == [1, 7]
    # the oracle in double: per-window probability and the state after every window
    model = vad_oracle.OracleSileroVAD({k: np.asarray(v, np.float64) for k, v in c["sd"].items()})
    model.h, model.c, model.context = model.h.double(), model.c.double(), model.context.double()
    every = FR.vad_stream(c["sd"], c["audio"], np.float64, state_after=tuple(range(1, W + 1)))
    for w in range(W):
        with torch.no_grad():
            x1 = torch.cat([model.context, torch.from_numpy(np.array(c["audio"][512 * w:512 * (w + 1)])).double()])
            p, model.h, model.c = vad_oracle.window_forward(model.sd, x1, model.h, model.c)
            model.context = x1[-64:]
        assert abs(float(p) - every["probs"][w]) <= 1e-12
        assert np.abs(model.h.numpy()[0] - every["states"][w + 1][0]).max() <= 1e-12
        assert np.abs(model.c.numpy()[0] - every["states"][w + 1][1]).max() <= 1e-12
    # the calls do not matter to the reference; the restatement passes its own rule
    cut = FR.vad_stream(c["sd"], c["audio"], np.float64, calls=c["calls"], state_after=c["state_after"])
    assert np.array_equal(cut["probs"], ref["probs"]) and np.array_equal(cut["h"], ref["h"])
    R, F32 = vad_outputs(ref, c["state_after"]), vad_outputs(f32, c["state_after"])
    allowed = {}
    for key in R:
        restatement_passes(R[key], F32[key], "vad")
        allowed[key] = FR.allowed_error(R[key], F32[key], "vad")
    for chunked in (False, True):
        for m in FC.vad_mutants(c, chunked):
            mu = vad_outputs(FR.vad_stream(c["sd"], c["audio"], np.float64, calls=c["calls"] if chunked else None, mutant=m,
                                           state_after=c["state_after"]), c["state_after"])
            ratios = {key: caught(mu[key], R[key], allowed[key])[1] for key in R}
            assert max(ratios.values()) > 1.0, f"{name} cannot tell '{m}' from the reference: {ratios}"
    # the forget gate is invisible after window 1 (c = 0 going in): only from window 2 on can the state show it
    assert set(FR.VAD_MUTANTS) - set(FC.vad_mutants(c, False)) == {"context_not_carried_between_calls"}


def test_the_random_vad_weights_meet_their_conditions():
    """from the float64 reference alone: every channel of every encoder layer is on in at least one window and off in at
    least one, every LSTM gate pre-activation is inside (-6, 6), every probability inside (0.05, 0.95)"""
    c, ref, _ = vad_refs("random")
    wins = FC.vad_windows(c["audio"])
    pre = [FR.vad_encoder(c["sd"], x1)[1] for x1 in wins]
    for layer in range(4):
        on = np.stack([(p[layer] > 0).any(axis=1) for p in pre])          # [W][C]: the channel passes something on
        assert on.any(axis=0).all() and (~on).any(axis=0).all(), (layer, int((~on.any(0)).sum()), int(on.all(0).sum()))
    assert np.abs(ref["gates"]).max() < 6.0
    assert 0.05 < ref["probs"].min() and ref["probs"].max() < 0.95
    assert ref["probs"].max() - ref["probs"].min() > 0.1                 # they move
    a = c["audio"].reshape(33, 512)
    assert sum(not w.any() for w in a) == 5 and np.abs(a[25:]).max() < 0.02


def test_the_real_vad_weights_are_the_production_magnitudes():
    c, ref, _ = vad_refs("real")
    assert max(np.abs(v).max() for k, v in c["sd"].items() if "basis" not in k) > 16.0
    assert np.abs(ref["gates"]).max() > 6.0
