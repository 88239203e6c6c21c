"""Plain numpy references of the three audio front ends: the Whisper log-mel (csrc/mel.hip: the streaming form behind
wlk_encode and the whole-file form wlk_log_mel), the generic mel-spectrogram of the diarization path (csrc/melspec.hip) and
the Silero VAD network with its context and state rules (csrc/vad.hip, oracle/vad_oracle.py).

Two statements of every operation, from the same float32 inputs (samples, window, filter bank, weights):
  * float64 (`dt=np.float64`): what the kernels are compared with;
  * float32 (`dt=np.float32`): the yardstick.  For the two spectrogram kernels it keeps the DFT as their headers state it -
    float32 windowed samples, the DFT accumulated in float64, its result rounded to float32, float32 from there on: the
    fp64 DFT is a design claim of these kernels and the suite holds them to it.  The VAD is float32 throughout, as its
    header says.  Its distance from the float64 form on a case is what the GPU test sizes its tolerance with, nothing else.
`mutant` names a deliberate mistake (tests/test_frontend_reference_cpu.py shows that every case it applies to tells it
from the reference); the GPU test never passes one.  No torch in here.

Tolerance (select_reference.value_tolerance, unchanged): a value may be off by KERNEL_FACTOR x the restatement's largest
error on the same case, floored at FLOOR * max(1, |reference|).  No element is left out: max, clamp and ReLU are
continuous.  FAMILY_FACTOR holds what a family needed beyond that on an MI355X, measured against float64."""
import numpy as np

from select_reference import FLOOR, KERNEL_FACTOR, abs_err, value_tolerance  # noqa: F401  (the rule lives there)

N_FFT, HOP, N_FREQ = 400, 160, 201
STREAM_PADDING, STREAM_FRAMES = 480000, 3000

LOG_MEL_MUTANTS = ("hann_symmetric", "reflect_repeats_edge", "right_reflect_off_by_one", "frame_shift_one_sample",
                   "bin0_dropped", "nyquist_dropped", "filter_last_tap_dropped", "filter_hole_skipped", "clamp_1e-9",
                   "floor_7_99")
MELSPEC_MUTANTS = ("preemph_first_sample", "window_left_aligned", "hann_periodic", "reflect_padding", "guard_dropped",
                   "nyquist_dropped")
VAD_MUTANTS = ("pad_edge_repeated", "pad_zero", "context_zero", "context_not_carried_between_calls", "bin128_dropped",
               "gate_order", "bias_hh_dropped", "no_relu_before_decoder", "tanh_c_dropped", "state_not_carried")

# what multiplies KERNEL_FACTOR for a family (1 = the unchanged rule), with the measured worst error / allowed it came from
FAMILY_FACTOR = {"log_mel": 1.0, "melspec": 1.0, "vad": 1.0}


def hann(n, periodic):
    """torch.hann_window(n, periodic) rounded to float32 - an INPUT of the kernels (the packed `mel.window`, the window
    wlk_melspec_create is given)"""
    k = np.arange(n, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * k / (n if periodic else n - 1))).astype(np.float32)


def _dft(frames, n_fft, dt):
    """frames [T][n_fft] (float64 values; float32-representable ones for the restatement) -> (re, im) [T][n_fft / 2 + 1]:
    X[k] = sum_n x[n] e^{-2 pi i k n / n_fft}, accumulated in float64 in both statements, rounded to float32 in the
    restatement."""
    k = np.arange(n_fft // 2 + 1)[None, :]
    n = np.arange(n_fft)[:, None]
    ang = 2.0 * np.pi * ((k * n) % n_fft).astype(np.float64) / n_fft          # the argument reduced exactly
    re = frames.astype(np.float64) @ np.cos(ang)
    im = -(frames.astype(np.float64) @ np.sin(ang))
    return re.astype(dt), im.astype(dt)


def _apply_bank(power, bank, dt, mutant):
    """power [T][n_freq], bank [n_mels][n_freq] float32 -> [T][n_mels]"""
    bank = np.array(bank, dtype=np.float32, copy=True)
    if mutant in ("filter_last_tap_dropped", "filter_hole_skipped"):
        for row in bank:
            nz = np.flatnonzero(row)
            if nz.size == 0:
                continue
            if mutant == "filter_last_tap_dropped":
                row[nz[-1]] = 0.0
            else:
                zeros = np.flatnonzero(row[nz[0]:nz[-1] + 1] == 0.0)
                if zeros.size:
                    row[nz[0] + zeros[0]:] = 0.0
    return (power.astype(dt) @ bank.astype(dt).T).astype(dt)


# ----------------------------------------------------------------------------------------------------------------------
# Whisper log-mel
# ----------------------------------------------------------------------------------------------------------------------
def log_mel_frames(n_samples, padding):
    """frames of the whole-file form: torch.stft's 1 + n / hop minus the dropped last one"""
    return (n_samples + padding) // HOP


def log_mel_parts(audio, bank, padding, dt=np.float64, window=None, mutant=None):
    """-> (mel energies [n_mels][frames], L = log10(max(mel, 1e-10)) [n_mels][frames], gmax) in dt"""
    x = np.concatenate([np.asarray(audio, np.float32).reshape(-1), np.zeros(int(padding), np.float32)])
    n = x.size
    assert n > N_FFT // 2, "the padded signal must be longer than the 200-sample reflection"
    w = hann(N_FFT, periodic=(mutant != "hann_symmetric")) if window is None or mutant == "hann_symmetric" \
        else np.asarray(window, np.float32)
    T = n // HOP
    j = HOP * np.arange(T)[:, None] - N_FFT // 2 + np.arange(N_FFT)[None, :]
    if mutant == "frame_shift_one_sample":
        j = j + 1
    left, right = j < 0, j >= n
    if mutant == "reflect_repeats_edge":
        j = np.where(left, -j - 1, np.where(right, 2 * n - 1 - j, j))
    elif mutant == "right_reflect_off_by_one":
        j = np.where(left, -j, np.where(right, 2 * n - 3 - j, j))
    else:
        j = np.where(left, -j, np.where(right, 2 * (n - 1) - j, j))           # reflect: the edge sample is not repeated
    frames = (x[j].astype(dt) * w.astype(dt)[None, :]).astype(dt)             # float32 product in the restatement
    live = np.any(frames != 0, axis=1)                                        # a frame of zeros has a spectrum of zeros
    re, im = _dft(frames[live], N_FFT, dt)
    power = np.zeros((T, N_FREQ), dt)
    if dt == np.float64:
        power[live] = re * re + im * im
    else:
        mag = np.hypot(re, im).astype(dt)                                     # stft(...).abs()
        power[live] = (mag * mag).astype(dt)                                  # ** 2
    if mutant == "bin0_dropped":
        power[:, 0] = 0
    if mutant == "nyquist_dropped":
        power[:, N_FREQ - 1] = 0
    mel = _apply_bank(power, bank, dt, mutant).T
    clamp = dt(1e-9) if mutant == "clamp_1e-9" else dt(1e-10)
    L = np.log10(np.maximum(mel, clamp), dtype=dt)
    return mel, L, L.max()


def log_mel(audio, bank, padding=0, dt=np.float64, window=None, mutant=None):
    """whisper/audio.py:log_mel_spectrogram(audio, n_mels, padding) -> [n_mels][(n + padding) / 160] in dt"""
    _, L, gmax = log_mel_parts(audio, bank, padding, dt, window, mutant)
    floor = gmax - (dt(7.99) if mutant == "floor_7_99" else dt(8.0))
    return ((np.maximum(L, floor) + dt(4.0)) / dt(4.0)).astype(dt)


def log_mel_streaming(audio, bank, dt=np.float64, window=None, mutant=None):
    """the mel the streaming path gives the encoder: 30 s of zeros behind the buffer, the first 3000 frames
    -> ([n_mels][3000], content_mel_len)"""
    full = log_mel(audio, bank, STREAM_PADDING, dt, window, mutant)
    return np.ascontiguousarray(full[:, :STREAM_FRAMES]), (full.shape[1] - STREAM_FRAMES) // 2


def log_mel_past_audio(n_samples, padding):
    """first frame whose 400 samples all lie in the zero padding (only where the right reflection cannot bring a sample
    back: padding >= 200); such a frame is exactly (max(-10, gmax - 8) + 4) / 4"""
    total = log_mel_frames(n_samples, padding)
    if padding < N_FFT // 2:
        return total
    return min(total, (n_samples + N_FFT // 2 + HOP - 1) // HOP if n_samples > 0 else 0)


# ----------------------------------------------------------------------------------------------------------------------
# the generic mel-spectrogram (NeMo FilterbankFeatures)
# ----------------------------------------------------------------------------------------------------------------------
def melspec(audio, bank, n_fft, win_length, hop, preemph, guard, dt=np.float64, window=None, mutant=None):
    """pre-emphasis (y[0] = x[0]) -> centred frames of the zero-padded signal -> a window of win_length centred in n_fft ->
    power -> bank [n_mels][n_fft / 2 + 1] -> log(. + guard).  -> [len / hop + 1][n_mels] in dt"""
    x = np.asarray(audio, np.float32).reshape(-1)
    n = x.size
    p = dt(np.float32(preemph))
    y = x.astype(dt)
    if float(preemph) != 0.0:
        y = np.concatenate([y[:1], (y[1:] - p * y[:-1]).astype(dt)])
        if mutant == "preemph_first_sample":
            y[0] = y[0] - p * y[0]
    w = hann(win_length, periodic=(mutant == "hann_periodic")) if window is None or mutant == "hann_periodic" \
        else np.asarray(window, np.float32)
    assert w.size == win_length
    wfull = np.zeros(n_fft, np.float32)
    wlo = 0 if mutant == "window_left_aligned" else (n_fft - win_length) // 2
    wfull[wlo:wlo + win_length] = w
    T = n // hop + 1
    j = hop * np.arange(T)[:, None] - n_fft // 2 + np.arange(n_fft)[None, :]
    if mutant == "reflect_padding":
        assert n > n_fft // 2
        jr = np.where(j < 0, -j, np.where(j >= n, 2 * (n - 1) - j, j))
        samples = y[np.clip(jr, 0, n - 1)]
    else:
        samples = np.where((j >= 0) & (j < n), y[np.clip(j, 0, n - 1)], dt(0))
    frames = (samples * wfull.astype(dt)[None, :]).astype(dt)
    re, im = _dft(frames, n_fft, dt)
    if dt == np.float64:
        power = re * re + im * im
    else:
        mag = np.sqrt(re * re + im * im, dtype=dt)
        power = (mag * mag).astype(dt)
    if mutant == "nyquist_dropped":
        power[:, n_fft // 2] = 0
    mel = _apply_bank(power, bank, dt, None)
    g = dt(0) if mutant == "guard_dropped" else dt(np.float32(guard))
    with np.errstate(divide="ignore"):
        return np.log(mel + g, dtype=dt)


# ----------------------------------------------------------------------------------------------------------------------
# Silero VAD (16 kHz): oracle/vad_oracle.py window_forward and the context / state rules of OracleSileroVAD
# ----------------------------------------------------------------------------------------------------------------------
VAD_CONTEXT, VAD_WINDOW, VAD_HID = 64, 512, 128
VAD_STRIDES = (1, 2, 2, 1)


def _sigmoid(x, dt):
    one = dt(1.0)
    return (one / (one + np.exp(-x, dtype=dt))).astype(dt)


def _conv1d_k3(x, w, b, stride, dt):
    """Conv1d(kernel 3, padding 1): x [Cin][T], w [Cout][Cin][3], b [Cout] -> pre-activation [Cout][(T - 1) / stride + 1]"""
    cin, T = x.shape
    xp = np.zeros((cin, T + 2), dt)
    xp[:, 1:T + 1] = x
    To = (T - 1) // stride + 1
    out = np.empty((w.shape[0], To), dt)
    for t in range(To):
        out[:, t] = (np.tensordot(w, xp[:, stride * t:stride * t + 3], axes=([1, 2], [0, 1])).astype(dt) + b).astype(dt)
    return out


def vad_encoder(sd, x1, dt=np.float64, mutant=None):
    """one window x1 = [64 context | 512 samples] -> (features [128], the four layers' pre-activations [C][frames])"""
    x1 = np.asarray(x1, np.float32).astype(dt)
    if mutant == "pad_edge_repeated":
        pad = x1[::-1][:64]
    elif mutant == "pad_zero":
        pad = np.zeros(64, dt)
    else:
        pad = x1[-2:-66:-1]                                                   # ReflectionPad1d((0, 64))
    xs = np.concatenate([x1, pad])
    basis = np.asarray(sd["stft.forward_basis_buffer"], np.float32)[:, 0, :].astype(dt)       # [258][256]
    frames = np.stack([xs[128 * t:128 * t + 256] for t in range(4)], axis=1)                  # [256][4]
    spec = (basis @ frames).astype(dt)
    mag = np.sqrt(spec[:129] ** 2 + spec[129:] ** 2, dtype=dt)
    if mutant == "bin128_dropped":
        mag[128] = 0
    y, pre = mag, []
    for i, stride in enumerate(VAD_STRIDES):
        w = np.asarray(sd[f"encoder.{i}.reparam_conv.weight"], np.float32).astype(dt)
        b = np.asarray(sd[f"encoder.{i}.reparam_conv.bias"], np.float32).astype(dt)
        z = _conv1d_k3(y, w, b, stride, dt)
        pre.append(z)
        y = np.maximum(z, dt(0))
    return y[:, 0], pre


def vad_cell(sd, feat, h, c, dt=np.float64, mutant=None):
    """LSTMCell -> ReLU -> Conv1d(128, 1, 1) -> sigmoid.  -> (probability, h', c', gate pre-activations [512])"""
    wih, whh, bih, bhh = (np.asarray(sd[f"decoder.rnn.{k}"], np.float32).astype(dt)
                          for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
    if mutant == "bias_hh_dropped":
        bhh = np.zeros_like(bhh)
    gates = (((wih @ feat).astype(dt) + bih) + ((whh @ h).astype(dt) + bhh)).astype(dt)
    i, f, g, o = gates.reshape(4, VAD_HID)
    if mutant == "gate_order":
        g, o = o, g                                                           # taken as (i, f, o, g)
    c2 = (_sigmoid(f, dt) * c + _sigmoid(i, dt) * np.tanh(g, dtype=dt)).astype(dt)
    h2 = (_sigmoid(o, dt) * (c2 if mutant == "tanh_c_dropped" else np.tanh(c2, dtype=dt))).astype(dt)
    dw = np.asarray(sd["decoder.decoder.2.weight"], np.float32).reshape(-1).astype(dt)
    db = np.asarray(sd["decoder.decoder.2.bias"], np.float32).reshape(-1).astype(dt)[0]
    r = h2 if mutant == "no_relu_before_decoder" else np.maximum(h2, dt(0))
    logit = dt(np.dot(dw, r)) + db
    return _sigmoid(np.asarray(logit, dt), dt), h2, c2, gates


def vad_stream(sd, audio, dt=np.float64, calls=None, mutant=None, state_after=()):
    """A fresh stream (zero context and state) over the windows of `audio` (a multiple of 512 float32 samples), cut into
    calls of `calls` windows (None: one call).  -> dict: probs [W], h / c [128] after the last window, states = {n: (h, c)
    after n windows}, gates [W][512]"""
    a = np.asarray(audio, np.float32).reshape(-1)
    assert a.size and a.size % VAD_WINDOW == 0
    W = a.size // VAD_WINDOW
    calls = [W] if calls is None else list(calls)
    assert sum(calls) == W
    starts = set(np.cumsum([0] + calls[:-1]).tolist())
    h, c = np.zeros(VAD_HID, dt), np.zeros(VAD_HID, dt)
    context = np.zeros(VAD_CONTEXT, np.float32)
    probs, gates, states = np.empty(W, dt), np.empty((W, 4 * VAD_HID), dt), {}
    for w in range(W):
        if mutant == "context_zero" or (mutant == "context_not_carried_between_calls" and w in starts):
            context = np.zeros(VAD_CONTEXT, np.float32)
        if mutant == "state_not_carried":
            h, c = np.zeros(VAD_HID, dt), np.zeros(VAD_HID, dt)
        x1 = np.concatenate([context, a[VAD_WINDOW * w:VAD_WINDOW * (w + 1)]])
        feat, _ = vad_encoder(sd, x1, dt, mutant)
        probs[w], h, c, gates[w] = vad_cell(sd, feat, h, c, dt, mutant)
        context = x1[-VAD_CONTEXT:]
        if w + 1 in state_after:
            states[w + 1] = (h.copy(), c.copy())
    return dict(probs=probs, h=h, c=c, states=states, gates=gates)


# ----------------------------------------------------------------------------------------------------------------------
def judge(name, got, ref, f32, family):
    """-> (report entry, failure text or None) for one output on one case, under the family's factor"""
    allowed, e32 = value_tolerance(ref, f32)
    allowed = allowed * FAMILY_FACTOR[family]
    err = abs_err(got, ref)
    worst = int(np.argmax(err - allowed))
    entry = dict(kernel_err=float(err.max()), restatement_err=e32, allowed=float(allowed.reshape(-1)[worst]),
                 of_allowed=float((err / allowed).max()))
    fail = None
    if not np.all(np.isfinite(np.asarray(got, np.float64))):
        fail = f"{name}: not finite"
    elif (err > allowed).any():
        fail = (f"{name}: error {err.reshape(-1)[worst]:.3e} > allowed {allowed.reshape(-1)[worst]:.3e} "
                f"(restatement {e32:.3e}) at flat index {worst}")
    return entry, fail


def allowed_error(ref, f32, family):
    return value_tolerance(ref, f32)[0] * FAMILY_FACTOR[family]
