"""Plain numpy references of the kernels of csrc/sortformer.hip (the attention the Sortformer blocks and the NLLB encoder
share, the sub-sampling stem's convolutions, the Conformer convolution core, the sigmoid head, the input assembly), for
wlk_diag_sf_kernel.

Two statements of every floating-point operation, from the same float32 inputs:
  * float64 (`dt=np.float64`): what the kernels are compared with;
  * float32 (`dt=np.float32`): numpy float32 throughout.  Its distance from the float64 form on a case is the yardstick
    the GPU test sizes its tolerance with, nothing else.
`mutant` names a deliberate mistake (tests/test_sf_kernel_reference_cpu.py shows that every case tells it from the
reference); the GPU test never passes one.  No torch in here.

Tolerance (select_reference.value_tolerance, unchanged): a value may be off by KERNEL_FACTOR x the restatement's largest
error on the same case, floored at FLOOR * max(1, |reference|)."""
import numpy as np

from select_reference import FLOOR, KERNEL_FACTOR, abs_err, value_tolerance  # noqa: F401  (the rule lives there)

ATTENTION_MUTANTS = ("rel_off_by_one", "drop_last_key", "swap_uv", "scale_content_only", "seg_neighbour")


def sub_len(n):
    """output length of a 3-tap stride-2 padding-1 convolution"""
    return (n - 1) // 2 + 1


def _sigmoid(x, dt):
    one = dt(1.0)
    return (one / (one + np.exp(-x, dtype=dt))).astype(dt)


# ----------------------------------------------------------------------------------------------------------------------
# attention
# ----------------------------------------------------------------------------------------------------------------------
def _one_sequence(q, k, v, scale, dt, pos, pos_row0, u, vb, mutant, extra):
    """q / k / v [T][H][dh] float32 -> [T][H][dh] in dt.  pos [rows][H][dh] or None; u / vb [H][dh] or None.
    extra = (k row, v row) [H][dh] of a neighbouring sequence (mutant seg_neighbour only)."""
    T, H, dh = q.shape
    out = np.zeros((T, H, dh), dt)
    sc = dt(np.float32(scale))
    if mutant == "swap_uv":
        u, vb = vb, u
    for h in range(H):
        qh = q[:, h].astype(dt)
        qu = qh + u[h].astype(dt) if u is not None else qh
        qv = qh + vb[h].astype(dt) if vb is not None else qh
        K, V = k[:, h].astype(dt), v[:, h].astype(dt)
        if extra is not None:
            K = np.concatenate([K, extra[0][h].astype(dt)[None]])
            V = np.concatenate([V, extra[1][h].astype(dt)[None]])
        n_keys = K.shape[0]
        s = qu @ K.T                                                            # [T][n_keys]
        if pos is not None:
            lo = pos_row0 - (T - 1)
            window = pos[lo:lo + 2 * T - 1, h].astype(dt)                       # rows pos_row0 - (T - 1) .. pos_row0 + (T - 1)
            m = qv @ window.T                                                   # [T][2 T - 1]
            idx = (T - 1) - np.arange(T)[:, None] + np.arange(n_keys)[None, :]  # pos_row0 - i + j, inside the window
            if mutant == "rel_off_by_one":
                idx = idx + 1
            bd = np.take_along_axis(m, np.clip(idx, 0, 2 * T - 2), axis=1)
            s = (s * sc + bd) if mutant == "scale_content_only" else (s + bd) * sc
        else:
            s = s * sc
        if mutant == "drop_last_key" and n_keys > 1:
            s, V = s[:, :-1], V[:-1]
        s = s.astype(dt)
        mx = s.max(axis=1, keepdims=True)
        e = np.exp(s - mx, dtype=dt)
        inv = dt(1.0) / e.sum(axis=1, keepdims=True, dtype=dt)
        out[:, h] = ((e @ V) * inv).astype(dt)
    return out


def owned_rows(rows, segs):
    """-> bool [rows]: the rows some sequence owns (all of them without segments)"""
    if segs is None:
        return np.ones(rows, bool)
    own = np.zeros(rows, bool)
    for a, n in segs:
        own[a:a + n] = True
    return own


def attention(q, k, v, scale, dt=np.float64, pos=None, pos_row0=0, bias_u=None, bias_v=None, segs=None, mutant=None):
    """s[i][j] = scale ((q_i + u) . k_j + (q_i + v) . pos[pos_row0 - i + j]); out[i] = softmax_j(s[i]) . V, per head.
    q / k / v [rows][H][dh]; segs = [(start, T)] independent sequences (None: rows [0, len(q)) are one).
    -> out [rows][H][dh] in dt, NaN in rows no sequence owns."""
    q, k, v = (np.asarray(a, np.float32) for a in (q, k, v))
    out = np.full(q.shape, np.nan, dt)
    spans = [(0, q.shape[0])] if segs is None else list(segs)
    for n, (a, T) in enumerate(spans):
        extra = None
        if mutant == "seg_neighbour" and len(spans) > 1:
            b = spans[n + 1][0] if n + 1 < len(spans) else spans[n - 1][0] + spans[n - 1][1] - 1
            extra = (k[b], v[b])
        out[a:a + T] = _one_sequence(q[a:a + T], k[a:a + T], v[a:a + T], scale, dt, pos, pos_row0, bias_u, bias_v,
                                     mutant, extra)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# ConvSubsampling('dw_striding'): conv0 and the depthwise stride-2 stages, sessions stacked along the time axis
# ----------------------------------------------------------------------------------------------------------------------
def _taps2d(x, dt, shift_centre):
    """x [T][F] or [T][F][C] -> the 9 taps of a 3x3 stride-2 padding-1 window, each [To][Fo](...)"""
    T, F = x.shape[:2]
    To, Fo = sub_len(T), sub_len(F)
    xp = np.zeros((2 * To + 3, 2 * Fo + 2) + x.shape[2:], dt)
    xp[1:T + 1, 1:F + 1] = x.astype(dt)
    taps = []
    for ky in range(3):
        for kx in range(3):
            t0 = ky + (1 if shift_centre and ky == 1 and kx == 1 else 0)       # the mutant: the centre tap one frame late
            taps.append(xp[t0:t0 + 2 * To:2, kx:kx + 2 * Fo:2])
    return taps


def _sessions(lens):
    a = 0
    for n in lens:
        yield a, n
        a += n


def conv0(x, w, b, lens, dt=np.float64, mutant=None):
    """Conv2d(1, C, 3, stride 2, padding 1) + ReLU per session: x [sum lens][F], w [C][9], b [C] -> [sum sub][sub(F)][C]"""
    w, b = np.asarray(w, np.float32).astype(dt), np.asarray(b, np.float32).astype(dt)
    outs = []
    for a, n in _sessions(lens):
        taps = _taps2d(np.asarray(x, np.float32)[a:a + n], dt, mutant == "tap_shifted")
        acc = np.zeros(taps[0].shape + (w.shape[0],), dt)
        for t in range(9):
            acc = (acc + taps[t][..., None] * w[:, t]).astype(dt)
        outs.append(np.maximum(acc + b, dt(0)).astype(dt))
    return np.concatenate(outs)


def dwconv2d(x, w, b, lens, dt=np.float64, mutant=None):
    """depthwise Conv2d(C, C, 3, stride 2, padding 1): x [sum lens][F][C], w tap-major [9][C], b [C]"""
    w, b = np.asarray(w, np.float32).astype(dt), np.asarray(b, np.float32).astype(dt)
    outs = []
    for a, n in _sessions(lens):
        taps = _taps2d(np.asarray(x, np.float32)[a:a + n], dt, mutant == "tap_shifted")
        acc = np.zeros(taps[0].shape, dt)
        for t in range(9):
            acc = (acc + taps[t] * w[t]).astype(dt)
        outs.append((acc + b).astype(dt))
    return np.concatenate(outs)


# ----------------------------------------------------------------------------------------------------------------------
# ConformerConvolution core
# ----------------------------------------------------------------------------------------------------------------------
def glu_dwconv(x, w, b, bn_mean, bn_invstd, bn_w, bn_b, lens, dt=np.float64, mutant=None):
    """GLU -> depthwise Conv1d(taps, same padding inside the session) -> BatchNorm1d(eval) -> Swish.
    x [sum lens][2 d], w [taps][d] -> [sum lens][d]"""
    x = np.asarray(x, np.float32).astype(dt)
    w, b, bn_mean, bn_invstd, bn_w, bn_b = (np.asarray(a, np.float32).astype(dt) for a in (w, b, bn_mean, bn_invstd, bn_w, bn_b))
    taps, d = w.shape
    half = (taps - 1) // 2
    if mutant == "bn_mean_sign":
        bn_mean = -bn_mean
    outs = []
    for a, n in _sessions(lens):
        glu = (x[a:a + n, :d] * _sigmoid(x[a:a + n, d:], dt)).astype(dt)
        gp = np.zeros((n + 2 * half + 1, d), dt)
        gp[half:half + n] = glu
        acc = np.zeros((n, d), dt)
        for t in range(taps):
            t0 = t + (1 if mutant == "tap_shifted" and t == half else 0)
            acc = (acc + gp[t0:t0 + n] * w[t]).astype(dt)
        y = ((acc + b - bn_mean) * bn_invstd * bn_w + bn_b).astype(dt)
        outs.append((y * _sigmoid(y, dt)).astype(dt))
    return np.concatenate(outs)


# ----------------------------------------------------------------------------------------------------------------------
# SortformerModules.forward_speaker_sigmoids (eval) and the encoder input
# ----------------------------------------------------------------------------------------------------------------------
def head(x, w1t, b1, w2, b2, dt=np.float64):
    """relu -> Linear + relu -> Linear -> sigmoid; w1t = the first Linear's weight transposed ([in][out])"""
    x, w1t, b1, w2, b2 = (np.asarray(a, np.float32).astype(dt) for a in (x, w1t, b1, w2, b2))
    h = np.maximum((np.maximum(x, dt(0)) @ w1t).astype(dt) + b1, dt(0)).astype(dt)
    return _sigmoid((h @ w2.T).astype(dt) + b2, dt)


def assemble(ctx_rows, chunk_rows, lens, chunk_lens, scale, dt=np.float64):
    """[context | chunk] * scale per session: ctx_rows [sum lens][d] holds the context rows at their stacked positions,
    chunk_rows [sum chunk_lens][d] the chunk rows in session order"""
    ctx_rows, chunk_rows = np.asarray(ctx_rows, np.float32), np.asarray(chunk_rows, np.float32)
    out = np.zeros(ctx_rows.shape, dt)
    c0 = 0
    for (a, n), nc in zip(_sessions(lens), chunk_lens):
        out[a:a + n - nc] = ctx_rows[a:a + n - nc].astype(dt)
        out[a + n - nc:a + n] = chunk_rows[c0:c0 + nc].astype(dt)
        c0 += nc
    return (out * dt(np.float32(scale))).astype(dt)


# ----------------------------------------------------------------------------------------------------------------------
def judge(name, got, ref, f32):
    """-> (report entry, failure text or None) for one output on one case"""
    allowed, e32 = value_tolerance(ref, f32)
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
