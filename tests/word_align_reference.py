"""Plain numpy statements of the device half of find_alignment (csrc/word_align.hip; the reference's whisper/timing.py:197-214).

Every stage twice, by one function with the number type as an argument:
  * float64: what the kernels are compared with;
  * float32: numpy float32 throughout (two-pass softmax, float32 mean and population std, float32 head sum).  Its distance
    from the float64 form on a case is the yardstick the GPU test sizes its tolerance with
    (select_reference.value_tolerance: 4 x that error, floor 2^-22 max(1, |reference|)), nothing else.
`cost_from_z` in float32 is also the kernel's arithmetic restated exactly - median by selection, heads added in ascending
order onto 0, one division, the negation - so on the kernel's own z it must give the kernel's cost bit for bit.

A NaN is ordered last by the median (np.sort, as torch.sort in the reference's `x.unfold(-1, 7, 1).sort()[0][..., 3]`).
`median7_dropping_nan` is the compare-exchange network wa_median7 had before it was changed to that order (fminf / fmaxf
return the other operand for a NaN); the CPU test keeps the disagreement on record.

`mistake` switches one deliberate error on (MISTAKES); test_word_align_reference_cpu.py requires that some named case tells
every one of them from the reference at the GPU test's tolerance.  No torch in here.

OUTPUT_FACTOR: families whose kernel-to-restatement factor is not the default 4, with the case that measured it (none so
far: every case of word_align_cases.py is held to 4)."""
import numpy as np

from select_reference import abs_err, value_tolerance

OUTPUT_FACTOR = {}

MISTAKES = ("sample_std", "edge_reflection", "median_index_4", "softmax_over_T", "scale_after_softmax", "row0_plus_1",
            "row0_minus_1", "head_sum_not_divided", "token_softmax_past_n_cols", "target_plus_1")


def token_prob(logits, n_cols, targets, dt=np.float64, mistake=None):
    """softmax(logits[i, :n_cols])[targets[i]]"""
    x = np.asarray(logits, np.float32)
    x = (x if mistake == "token_softmax_past_n_cols" else x[:, :n_cols]).astype(dt)
    t = np.asarray(targets, np.int64)
    if mistake == "target_plus_1":
        t = (t + 1) % n_cols
    mx = x.max(axis=1, keepdims=True)
    e = np.exp(x - mx, dtype=dt)
    return (e[np.arange(len(t)), t] / e.sum(axis=1, dtype=dt)).astype(dt)


def softmax(ring, P, F, qk_scale, dt=np.float64, mistake=None):
    """ring [A][ring_rows][T] raw scores -> w [A][P][F] = softmax(qk_scale * ring[:, :P, :F]) over the frames"""
    cut = ring.shape[2] if mistake == "softmax_over_T" else F
    x = np.asarray(ring, np.float32)[:, :P, :cut].astype(dt)
    s = dt(qk_scale)
    if mistake != "scale_after_softmax":
        x = x * s
    with np.errstate(invalid="ignore"):
        mx = x.max(axis=2, keepdims=True)
        e = np.exp(x - mx, dtype=dt)
        w = e / e.sum(axis=2, keepdims=True, dtype=dt)
    if mistake == "scale_after_softmax":
        w = w * s
    return w[:, :, :F].astype(dt)


def zscore(w, dt=np.float64, mistake=None):
    """(w - mean) / std over the token axis: population std, no epsilon (0 / 0 = NaN for a constant column)"""
    w = np.asarray(w).astype(dt)
    P = w.shape[1]
    mean = w.mean(axis=1, keepdims=True, dtype=dt)
    t = w - mean
    var = (t * t).sum(axis=1, keepdims=True, dtype=dt) / dt(P - 1 if mistake == "sample_std" else P)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (t / np.sqrt(var, dtype=dt)).astype(dt)


def _window_index(F, mistake=None):
    idx = np.arange(-3, F + 3)
    if mistake == "edge_reflection":
        return np.clip(idx, 0, F - 1)
    idx = np.abs(idx)
    return np.where(idx >= F, 2 * (F - 1) - idx, idx)


def median7(z, mistake=None):
    """width-7 median along the frames, reflect padding; rows of at most 3 frames are left as they are"""
    F = z.shape[-1]
    if F <= 3:
        return z
    win = np.lib.stride_tricks.sliding_window_view(z[..., _window_index(F, mistake)], 7, axis=-1)
    return np.sort(win, axis=-1)[..., 4 if mistake == "median_index_4" else 3]


def median7_dropping_nan(z):
    """the insertion network on fminf / fmaxf (minNum / maxNum: a NaN operand is dropped), as wa_median7 was"""
    F = z.shape[-1]
    if F <= 3:
        return z
    win = np.lib.stride_tricks.sliding_window_view(z[..., _window_index(F)], 7, axis=-1)
    v = [win[..., i].copy() for i in range(7)]
    for i in range(1, 7):
        for j in range(i, 0, -1):
            lo, hi = np.fmin(v[j - 1], v[j]), np.fmax(v[j - 1], v[j])
            v[j - 1], v[j] = lo, hi
    return v[3]


def cost_from_z(z, n_sot, dt=np.float64, mistake=None):
    """z [A][P][F] -> cost [P - n_sot - 1][F] = -(sum over the heads in ascending order) / A of the rows n_sot .. P - 2"""
    z = np.asarray(z).astype(dt)
    A, P, F = z.shape
    row0 = n_sot + (1 if mistake == "row0_plus_1" else -1 if mistake == "row0_minus_1" else 0)
    N = P - n_sot - 1
    acc = np.zeros((N, F), dt)
    with np.errstate(invalid="ignore"):
        for a in range(A):                  # (one head at a time: the windows of 10 x 448 x 1500 would be 380 MB)
            acc = acc + median7(z[a, row0:row0 + N], mistake)
        return (-(acc if mistake == "head_sum_not_divided" else acc / dt(A))).astype(dt)


def chain(case, dt=np.float64, mistake=None):
    """every stage's result for a case of word_align_cases.py: probs [n_text], w, z [A][P][F], cost [n_text + 1][F]"""
    c = case
    w = softmax(c["ring"], c["P"], c["F"], c["qk_scale"], dt, mistake)
    z = zscore(w, dt, mistake)
    return dict(probs=token_prob(c["logits"], c["n_cols"], c["targets"], dt, mistake), w=w, z=z,
                cost=cost_from_z(z, c["n_sot"], dt, mistake))


def compare(ref, f32, got, keys=("probs", "w", "z", "cost")):
    """`got` (the kernels' outputs, or a deliberately wrong statement) against the float64 results `ref`, key by key, with
    the float32 restatement `f32` sizing the tolerance.  -> (report, failures).  A NaN must stand exactly where the
    reference has one (abs_err: a NaN beside a number is an infinite error)."""
    report, failures = {}, []
    for key in keys:
        if key not in got:
            continue
        allowed, e32 = value_tolerance(ref[key], f32[key])
        err = abs_err(got[key], ref[key])
        worst = int(np.argmax(err - allowed))
        report[key] = dict(restatement_err=e32, kernel_err=float(err.max()), allowed=float(allowed.reshape(-1)[worst]),
                           ratio=float(err.max() / e32) if e32 > 0 else None)
        if (err > allowed).any():
            failures.append(f"{key}: error {err.reshape(-1)[worst]:.3e} > allowed {allowed.reshape(-1)[worst]:.3e} "
                            f"(restatement {e32:.3e}) at flat index {worst}")
    return report, failures
