"""Inputs of the audio front-end tests: one generator module for test_frontend_reference_cpu.py (which checks the
references of tests/frontend_reference.py and the cases' power to tell mistakes apart) and test_gpu_frontend.py (which
runs them through wlk_encode, wlk_log_mel, wlk_melspec_run and wlk_vad_*).  Everything is seeded by name; the only files
read are the Silero DFT basis and, for one case, the real checkpoint (tests/golden/vad_weights_16k.npz).

What the production inputs never reach, and these do: filter rows with weight on bin 0 and on the Nyquist bin, a row
over all bins, an empty row, a row with a hole in its support (the sparse extents filt_lo / filt_hi); energies under the
1e-10 clamp with the max - 8 floor below it; the whole-file form with 128 bins, with every padding at which its code takes
another path and at the smallest length it accepts; mel-spectrogram settings other than NeMo's; VAD weights under which
every encoder channel switches on and off, no gate saturates and no probability sits on the flat of the sigmoid."""
import functools
import os
import zlib

import numpy as np

import frontend_reference as FR
from whisperlivekit_amd import synth
from whisperlivekit_amd.melbank import mel_filterbank

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ----------------------------------------------------------------------------------------------------------------------
# signals (float32, 0.2 - 1.5 s at 16 kHz)
# ----------------------------------------------------------------------------------------------------------------------
QUIET_GAIN = np.float32(1e-3)


@functools.lru_cache(maxsize=None)
def signal(kind, n=None):
    if kind == "speech":
        a = synth.to_pcm16_roundtrip(synth.speech_like(1.5, 21))
    elif kind == "noise":
        a = synth.to_pcm16_roundtrip(synth.white_noise(1.0, 22))
    elif kind == "dc_tone":                   # an offset and a tone on the centre of DFT bin 25 (400-point) / 32 (512-point)
        t = np.arange(8000, dtype=np.float64)
        a = (0.25 + 0.5 * np.sin(2.0 * np.pi * 1000.0 * t / 16000.0 + 0.3)).astype(np.float32)
    elif kind == "impulse":                   # inside the first 200 samples: frame 0 sees it twice, once reflected
        a = np.zeros(4800, np.float32)
        a[100] = 1.0
    elif kind == "square":                    # full scale, 800 Hz
        a = np.where((np.arange(4800) // 10) % 2 == 0, 1.0, -1.0).astype(np.float32)
    elif kind == "bursts":                    # digital silence between two bursts
        a = np.concatenate([signal("noise")[:3200], np.zeros(6400, np.float32), signal("speech")[2000:6800]])
    elif kind == "quiet":                     # float32 scaling, no int16 round trip: 16 levels would be left of it
        a = (synth.speech_like(1.0, 23) * QUIET_GAIN).astype(np.float32)
    elif kind == "zeros":
        a = np.zeros(3200, np.float32)
    else:
        raise KeyError(kind)
    a = np.ascontiguousarray(a[:n] if n is not None else a, np.float32)
    assert n is None or a.size == n, (kind, n)
    a.setflags(write=False)
    return a


# ----------------------------------------------------------------------------------------------------------------------
# filter banks, all with non-negative weights
# ----------------------------------------------------------------------------------------------------------------------
EDGE_ROWS = dict(bin0=0, nyquist=1, low4=2, all_bins=3, empty=4, hole=5)


@functools.lru_cache(maxsize=None)
def bank(kind, n_mels, n_fft=400):
    """'slaney': the production bank.  'edges': its rows 0 .. 5 replaced by a row with its only tap on bin 0, one with its
    only tap on the Nyquist bin, one over bins 0 .. 3, one over all bins, an empty one and one with two zeros inside its
    support; the slaney rows for the rest."""
    b = np.array(mel_filterbank(n_mels, 16000, n_fft), dtype=np.float32, copy=True)
    nf = n_fft // 2 + 1
    if kind == "edges":
        rng = _rng(f"edges{n_mels}_{n_fft}")
        b[:6] = 0.0
        b[0, 0] = 0.02
        b[1, nf - 1] = 0.02
        b[2, :4] = [0.01, 0.02, 0.015, 0.005]
        b[3] = (0.0005 + 0.002 * rng.random(nf)).astype(np.float32)
        b[5, 50:61] = (0.005 + 0.01 * rng.random(11)).astype(np.float32)
        b[5, 54:56] = 0.0
    else:
        assert kind == "slaney"
    assert (b >= 0).all()
    b.setflags(write=False)
    return b


# ----------------------------------------------------------------------------------------------------------------------
# Whisper log-mel, whole-file form: name -> (signal, n_samples, padding, bank, n_mels)
# ----------------------------------------------------------------------------------------------------------------------
LOG_MEL = {
    "speech_16000_p0_slaney80": ("speech", 16000, 0, "slaney", 80),           # 100 frames, all active
    "noise_10240_p0_edges128": ("noise", 10240, 0, "edges", 128),             # 64 frames: one full tile of the finish
    "speech_3999_p1_edges80": ("speech", 3999, 1, "edges", 80),               # the reflection passes one zero
    "noise_4120_p40_slaney128": ("noise", 4120, 40, "slaney", 128),           # ... reads one last real sample
    "noise_4119_p41_edges128": ("noise", 4119, 41, "edges", 128),             # ... and none
    "noise_4060_p100_slaney128": ("noise", 4060, 100, "slaney", 128),
    "bursts_14400_p199_edges128": ("bursts", 14400, 199, "edges", 128),       # the last padding that computes every frame
    "square_4800_p200_edges80": ("square", 4800, 200, "edges", 80),           # the first that leaves frames to the fill
    "dc_tone_6400_p480000_slaney80": ("dc_tone", 6400, 480000, "slaney", 80),
    "speech_16000_p480000_edges128": ("speech", 16000, 480000, "edges", 128),
    "impulse_4800_p0_edges80": ("impulse", 4800, 0, "edges", 80),
    "dc_tone_8000_p0_edges128": ("dc_tone", 8000, 0, "edges", 128),
    "quiet_16000_p0_edges128": ("quiet", 16000, 0, "edges", 128),
    "quiet_16000_p480000_slaney80": ("quiet", 16000, 480000, "slaney", 80),
    "noise_201_p0_edges128": ("noise", 201, 0, "edges", 128),                 # n + padding = 201: one frame
    "noise_1_p200_slaney80": ("noise", 1, 200, "slaney", 80),
    "zeros_3200_p0_slaney128": ("zeros", 3200, 0, "slaney", 128),             # every energy under the clamp
    "zeros_3200_p1000_edges80": ("zeros", 3200, 1000, "edges", 80),
    "empty_0_p1000_slaney128": ("zeros", 0, 1000, "slaney", 128),             # no sample at all: no frame kernel runs
}
LOG_MEL_NAMES = list(LOG_MEL)
LOG_MEL_REFUSED = ((200, 0), (0, 200), (100, 100), (1, 0))                    # n + padding <= 200


def log_mel_case(name):
    kind, n, padding, bk, n_mels = LOG_MEL[name]
    return dict(name=name, signal=kind, audio=signal(kind, n), padding=padding, bank_kind=bk, n_mels=n_mels,
                bank=bank(bk, n_mels), streaming=False)


# streaming form: name -> (bank, n_mels, script).  Script steps: ("append", signal, lo, hi), ("pcm16", signal, lo, hi),
# ("drop", n), ("encode",); the mel of the LAST encode is the case's output, the buffer at that point its input.
STREAM = {
    "pieces_speech_slaney80": ("slaney", 80, (("append", "speech", 0, 100), ("encode",), ("append", "speech", 100, 4100),
                                              ("encode",), ("append", "speech", 4100, 16000), ("encode",))),
    # an eviction of whole frames between two encodes: the two head frames are recomputed, the left reflection is live
    "drop_front_speech_edges128": ("edges", 128, (("append", "speech", 0, 12000), ("encode",), ("drop", 3200),
                                                  ("append", "speech", 12000, 19000), ("encode",))),
    "drop_front_unaligned_noise_edges80": ("edges", 80, (("append", "noise", 0, 9000), ("encode",), ("drop", 3333),
                                                         ("append", "noise", 9000, 12000), ("encode",))),
    "pcm16_bursts_slaney128": ("slaney", 128, (("pcm16", "bursts", 0, 5000), ("encode",), ("pcm16", "bursts", 5000, 14400),
                                               ("encode",))),
    "quiet_edges80": ("edges", 80, (("append", "quiet", 0, 8000), ("encode",), ("append", "quiet", 8000, 16000), ("encode",))),
    "square_edges128": ("edges", 128, (("append", "square", 0, 4800), ("encode",))),
}
STREAM_NAMES = list(STREAM)


def to_pcm16(a):
    return np.clip(np.round(np.asarray(a, np.float64) * 32768.0), -32768, 32767).astype(np.int16)


def stream_case(name):
    """-> dict with `audio`: the buffer the last encode sees (float32), as the reference's input"""
    bk, n_mels, script = STREAM[name]
    buf = np.zeros(0, np.float32)
    for step in script:
        if step[0] == "append":
            buf = np.concatenate([buf, signal(step[1])[step[2]:step[3]]])
        elif step[0] == "pcm16":
            buf = np.concatenate([buf, to_pcm16(signal(step[1])[step[2]:step[3]]).astype(np.float32) / np.float32(32768.0)])
        elif step[0] == "drop":
            buf = buf[step[1]:]
    sig = next(s[1] for s in script if s[0] in ("append", "pcm16"))
    return dict(name=name, signal=sig, audio=np.ascontiguousarray(buf, np.float32), padding=FR.STREAM_PADDING, bank_kind=bk,
                n_mels=n_mels, bank=bank(bk, n_mels), script=script, streaming=True)


def right_reflection_reach(n_samples, padding):
    """how many samples past the end of the padded signal the last kept frame reads (<= 40: torch.stft's own last frame is
    dropped), and how many of the samples the reflection brings back are real ones"""
    n = n_samples + padding
    T = n // FR.HOP
    reach = max(0, FR.HOP * (T - 1) + FR.N_FFT // 2 - n) if T else 0          # indices n .. n + reach - 1
    lowest = n - 1 - reach                                                    # reflected to n - 2 .. n - 1 - reach
    return reach, max(0, min(reach, n_samples - lowest))


def log_mel_mutants(case, ref_parts):
    """the mistakes of FR.LOG_MEL_MUTANTS this case can tell from the reference.  `ref_parts` = FR.log_mel_parts of the
    case in float64 (the energies, L and its maximum): the rules below read the case's inputs and the float64 reference,
    never a mutant's output.
      * nothing applies to a signal of zeros except the clamp;
      * the two reflection mistakes need a sample where they look: the left reflection reads samples 1 .. 200 (0 .. 199
        when the edge is repeated) under window taps 199 .. 0, so any sound in the first 201 samples shows; the right
        reflection reaches at most 40 samples past the end, under taps 360 .. 399 (weights below 0.1, falling to 6e-5):
        it shows only when most of those are real samples (padding <= 1) and the signal's last 40 samples are not silent;
      * bin 0 / the Nyquist bin / the hole need the `edges` bank (the slaney bank has no weight there);
      * `clamp_1e-9` needs an energy under 1e-9 above the floor: max L - 8 < -9;
      * `floor_7_99` needs a dynamic range above 8: some L under max L - 8."""
    mel, L, gmax = ref_parts
    audio = case["audio"]
    out = []
    silent = not np.any(audio)
    reach, real = right_reflection_reach(audio.size, case["padding"])
    left = bool(np.any(audio[:201]))
    right = real >= 30 and bool(np.any(audio[-40:]))
    if not silent:
        out += ["hann_symmetric", "frame_shift_one_sample", "filter_last_tap_dropped"]
        if left or right:
            out.append("reflect_repeats_edge")
        if right:
            out.append("right_reflect_off_by_one")
        if case["bank_kind"] == "edges":
            out += ["bin0_dropped", "nyquist_dropped", "filter_hole_skipped"]
    if gmax - 8.0 < -9.0 - 1e-3 and (mel < 0.5e-9).any():
        out.append("clamp_1e-9")
    if (L < gmax - 8.0).any():
        out.append("floor_7_99")
    return out


# ----------------------------------------------------------------------------------------------------------------------
# mel-spectrogram: name -> (n_fft, win_length, hop, n_mels, preemph, guard, bank, signal, n_samples)
# ----------------------------------------------------------------------------------------------------------------------
NEMO_GUARD = 2.0 ** -24
MELSPEC = {
    "nemo_speech": (512, 400, 160, 128, 0.97, NEMO_GUARD, "slaney", "speech", 16000),
    "nemo_edges_noise": (512, 400, 160, 128, 0.97, NEMO_GUARD, "edges", "noise", 12345),
    "nemo_edges_bursts": (512, 400, 160, 128, 0.97, NEMO_GUARD, "edges", "bursts", 14400),
    "nemo_short_200": (512, 400, 160, 128, 0.97, NEMO_GUARD, "edges", "speech", 200),        # shorter than n_fft / 2
    "nemo_one_sample": (512, 400, 160, 128, 0.97, NEMO_GUARD, "slaney", "noise", 1),
    "nemo_quiet": (512, 400, 160, 128, 0.97, NEMO_GUARD, "edges", "quiet", 8000),
    "nemo_dc_tone": (512, 400, 160, 128, 0.97, NEMO_GUARD, "edges", "dc_tone", 8000),
    "nemo_impulse": (512, 400, 160, 128, 0.97, NEMO_GUARD, "edges", "impulse", 4800),
    "f256_w200_h80_m40_square": (256, 200, 80, 40, 0.97, NEMO_GUARD, "slaney", "square", 4800),
    "f256_w200_h80_m40_edges_speech": (256, 200, 80, 40, 0.97, NEMO_GUARD, "edges", "speech", 8000),
    "full_window_f400_speech": (400, 400, 160, 80, 0.97, NEMO_GUARD, "edges", "speech", 8000),   # win_length == n_fft
    "odd_gap_f512_w401_noise": (512, 401, 160, 128, 0.97, NEMO_GUARD, "edges", "noise", 8000),   # n_fft - win_length odd
    "m256_f512_speech": (512, 400, 160, 256, 0.97, NEMO_GUARD, "edges", "speech", 8000),
    "no_preemph_speech": (512, 400, 160, 128, 0.0, NEMO_GUARD, "edges", "speech", 8000),
    "guard_1e-5_noise": (512, 400, 100, 64, 0.5, 1e-5, "edges", "noise", 5000),
}
MELSPEC_NAMES = list(MELSPEC)


def melspec_case(name):
    n_fft, win, hop, n_mels, preemph, guard, bk, kind, n = MELSPEC[name]
    return dict(name=name, n_fft=n_fft, win_length=win, hop=hop, n_mels=n_mels, preemph=preemph, guard=guard, bank_kind=bk,
                bank=bank(bk, n_mels, n_fft), signal=kind, audio=signal(kind, n), window=FR.hann(win, periodic=False))


def melspec_args(c):
    return (c["audio"], c["bank"], c["n_fft"], c["win_length"], c["hop"], c["preemph"], c["guard"])


def melspec_mutants(case):
    """the mistakes of FR.MELSPEC_MUTANTS this case can tell from the reference:
      * the first sample's pre-emphasis needs pre-emphasis and a first sample;
      * the window's place needs win_length < n_fft;
      * reflect padding needs a signal longer than n_fft / 2 (it is not defined below that) with sound near an end;
      * the Nyquist bin needs the `edges` bank."""
    c = case
    a = c["audio"]
    out = ["hann_periodic", "guard_dropped"]
    if c["preemph"] != 0.0 and a[0] != 0.0:
        out.append("preemph_first_sample")
    if c["win_length"] < c["n_fft"]:
        out.append("window_left_aligned")
    half = c["n_fft"] // 2
    if a.size > half and (np.any(a[1:half]) or np.any(a[-half:-1])):
        out.append("reflect_padding")
    if c["bank_kind"] == "edges":
        out.append("nyquist_dropped")
    return out


# ----------------------------------------------------------------------------------------------------------------------
# Silero VAD
# ----------------------------------------------------------------------------------------------------------------------
VAD_SHAPES = {
    "encoder.0.reparam_conv.weight": (128, 129, 3), "encoder.1.reparam_conv.weight": (64, 128, 3),
    "encoder.2.reparam_conv.weight": (64, 64, 3), "encoder.3.reparam_conv.weight": (128, 64, 3),
    "decoder.rnn.weight_ih": (512, 128), "decoder.rnn.weight_hh": (512, 128), "decoder.decoder.2.weight": (1, 128, 1),
}
VAD_SEED = "vad-random-0"
VAD_CALLS = (1, 7)                  # then the rest
VAD_STATE_AFTER = (1, 2)            # and after all windows


@functools.lru_cache(maxsize=None)
def real_vad_weights():
    with np.load(os.path.join(GOLDEN, "vad_weights_16k.npz")) as z:
        return {k: np.asarray(z[k], np.float32) for k in z.files}


@functools.lru_cache(maxsize=None)
def vad_audio():
    """33 windows: speech, exact silence, noise, speech at 0.02 gain"""
    sp = synth.to_pcm16_roundtrip(synth.speech_like(1.0, 31))
    a = np.concatenate([sp[2000:2000 + 12 * 512], np.zeros(5 * 512, np.float32),
                        synth.to_pcm16_roundtrip(synth.white_noise(0.3, 32))[:8 * 512],
                        (sp[8000:8000 + 8 * 512] * np.float32(0.02)).astype(np.float32)]).astype(np.float32)
    assert a.size == 33 * 512
    a.setflags(write=False)
    return a


def vad_windows(audio):
    """[W][576]: every window behind the 64 samples in front of it (zeros in front of the first)"""
    a = np.concatenate([np.zeros(64, np.float32), np.asarray(audio, np.float32)])
    return np.stack([a[512 * w:512 * w + 576] for w in range(audio.size // 512)])


@functools.lru_cache(maxsize=None)
def random_vad_weights(seed=VAD_SEED):
    """Every tensor but the DFT basis drawn at 1.4 / sqrt(fan_in); then, layer by layer, each encoder bias = minus the
    median over the case's windows of the channel's largest float64 pre-activation (so the channel is on in about half
    of the windows and off in the others); the decoder weight times 8 (probabilities that move)."""
    rng = _rng(seed)
    sd = {"stft.forward_basis_buffer": real_vad_weights()["stft.forward_basis_buffer"]}
    for k, shape in VAD_SHAPES.items():
        fan_in = int(np.prod(shape[1:]))
        sd[k] = (1.4 / np.sqrt(fan_in) * rng.standard_normal(shape)).astype(np.float32)
    for i in range(4):
        sd[f"encoder.{i}.reparam_conv.bias"] = np.zeros(VAD_SHAPES[f"encoder.{i}.reparam_conv.weight"][0], np.float32)
    sd["decoder.rnn.bias_ih"] = (0.1 * rng.standard_normal(512)).astype(np.float32)
    sd["decoder.rnn.bias_hh"] = (0.1 * rng.standard_normal(512)).astype(np.float32)
    sd["decoder.decoder.2.bias"] = (0.1 * rng.standard_normal(1)).astype(np.float32)
    sd["decoder.decoder.2.weight"] = (sd["decoder.decoder.2.weight"] * np.float32(8.0)).astype(np.float32)
    wins = vad_windows(vad_audio())
    for i in range(4):
        top = np.stack([FR.vad_encoder(sd, x1)[1][i].max(axis=1) for x1 in wins])      # [W][C], bias i still 0
        sd[f"encoder.{i}.reparam_conv.bias"] = (-np.median(top, axis=0)).astype(np.float32)
    for v in sd.values():
        v.setflags(write=False)
    return sd


VAD = {"random": ("random", None), "real": ("real", None)}
VAD_NAMES = list(VAD)


def vad_case(name):
    sd = random_vad_weights() if name == "random" else real_vad_weights()
    audio = vad_audio()
    W = audio.size // 512
    return dict(name=name, sd=sd, audio=audio, n_windows=W, calls=list(VAD_CALLS) + [W - sum(VAD_CALLS)],
                state_after=VAD_STATE_AFTER + (W,))


def vad_mutants(case, chunked):
    """the mistakes of FR.VAD_MUTANTS a run of the case can tell from the reference: all of them, except that the context
    can only be lost between calls when there is more than one call"""
    return [m for m in FR.VAD_MUTANTS if chunked or m != "context_not_carried_between_calls"]
