"""Cases and the float64 reference for the NLLB alignment read-out kernel alone (wlk_diag_nllb_align; csrc/nllb.hip
nllb_align_readout_kernel).  The GPU test (tests/test_gpu_nllb_alignatt.py) runs the kernel on them; the CPU test
(tests/test_nllb_alignatt.py) runs the float32 restatement of tests/nllb_align_standin.py through the same comparison.

Tolerance (select_reference.value_tolerance): a value may be off by 4 x the error the float32 restatement has on the same
case, floored at 2^-22 * max(1, |reference|).  The position equals the reference wherever the reference's margin over the
best other position of the window is an exact tie (0: the lowest position wins) or exceeds twice that allowance; the rows
in between are exempt - none of a planted case, at most 2 % of the random rows of a shape."""
import numpy as np

import select_reference as SR
from nllb_align_standin import readout

# (n_align, rows, S): one position, fewer positions than a wave, both sides of 64 / 256 (one and two positions per thread),
# the largest row; 1, 2, 3, 16, 32 and 64 heads; 1 to 8 rows
SHAPES = [(1, 1, 1), (1, 1, 2), (2, 1, 3), (16, 1, 63), (16, 2, 64), (32, 8, 65), (3, 1, 255), (16, 1, 256), (64, 8, 257),
          (16, 4, 512)]


def random_probs(n_align, rows, S, seed):
    """softmax rows of float32 logits ~ N(0, 2^2), as the cross-attention kernel leaves them"""
    x = (np.random.default_rng(seed).standard_normal((n_align, rows, S)) * 2).astype(np.float32)
    e = np.exp(x - x.max(axis=-1, keepdims=True), dtype=np.float32)
    return (e / e.sum(axis=-1, keepdims=True, dtype=np.float32)).astype(np.float32)


def cases_of(si):
    """-> [(name, kind, probs, lo, hi, limit)] for SHAPES[si]; kind is 'random' or 'planted'"""
    n, rows, S = SHAPES[si]
    base = random_probs(n, rows, S, 100 + si)
    lo, hi = 1, S - 1                                   # the content window ([1, 0) for S = 1: empty)
    out = [("content_limit0", "random", base, lo, hi, 0), ("whole_row_limit_inside", "random", base, 0, S, S // 2),
           ("content_limit_S", "random", base, lo, hi, S), ("empty_window", "planted", base, min(2, S), min(2, S), S // 3),
           ("inverted_window", "planted", base, S, 0, 0), ("one_element", "planted", base, S // 2, S // 2 + 1, 1 % (S + 1))]

    def planted(name, winner, decoys, lo, hi, limit):
        p = base.copy()
        p[:, :, winner] = np.float32(0.75)              # the same value in every head: the same float32 sum anywhere
        for j in decoys:
            p[:, :, j] = np.float32(0.875)              # larger, but outside the window: must be ignored
        out.append((name, "planted", p, lo, hi, limit))

    if S >= 5:
        lo2, hi2 = 2, S - 2
        planted("max_at_lo", lo2, [], lo2, hi2, 0)
        planted("max_at_hi_minus_1", hi2 - 1, [], lo2, hi2, S)
        planted("max_at_hi_ignored", (lo2 + hi2) // 2, [hi2], lo2, hi2, hi2)
        planted("max_at_0_ignored", hi2 - 1, [0], lo2, hi2, 1)
        planted("both_sides_ignored", lo2, [0, 1, hi2, S - 1], lo2, hi2, S - 1)
        tie = base.copy()                               # exact ties: the lowest position wins
        for j in {lo2, (lo2 + hi2) // 2, hi2 - 1, hi2, 0}:
            tie[:, :, j] = np.float32(0.75)
        out.append(("tie_lowest_wins", "planted", tie, lo2, hi2, 0))
        tie2 = base.copy()
        for j in {(lo2 + hi2) // 2, hi2 - 1}:
            tie2[:, :, j] = np.float32(0.75)
        out.append(("tie_of_two", "planted", tie2, 0, S, S // 2))
    return out


def reference(probs, lo, hi, limit):
    """float64 -> (p [rows, S], pos [rows], prob [rows], mass [rows], margin [rows]); margin = winner minus the best other
    position of the window (0 = exact tie, inf = a window of one or none)"""
    x = np.asarray(probs, np.float32).astype(np.float64)
    n, rows, S = x.shape
    p = x.sum(axis=0) / n
    lo, hi = max(lo, 0), min(hi, S)
    pos = np.full(rows, -1, np.int64)
    prob = np.zeros(rows)
    margin = np.full(rows, np.inf)
    for r in range(rows):
        if hi > lo:
            w = p[r, lo:hi]
            a = int(np.argmax(w))
            pos[r], prob[r] = lo + a, w[a]
            if len(w) > 1:
                margin[r] = w[a] - np.delete(w, a).max()
    return p, pos, prob, p[:, limit:].sum(axis=1), margin


def compare(kind, probs, lo, hi, limit, got):
    """got = (p, pos, prob, mass) of the kernel (or of the restatement) -> (report, failures, exempt rows, rows)"""
    ref_p, ref_pos, ref_prob, ref_mass, margin = reference(probs, lo, hi, limit)
    f32_p, f32_pos, f32_prob, f32_mass = readout(probs, lo, hi, limit)
    got_p, got_pos, got_prob, got_mass = got
    failures, report = [], {}
    tol_p, e32 = SR.value_tolerance(ref_p, f32_p)
    for key, ref, f32, val in (("p", ref_p, f32_p, got_p), ("mass", ref_mass, f32_mass, got_mass)):
        allowed, e = SR.value_tolerance(ref, f32)
        err = SR.abs_err(val, ref)
        report[key] = dict(kernel_err=float(err.max()), restatement_err=e, allowed=float(allowed.max()))
        if (err > allowed).any():
            failures.append(f"{key}: error {err.max():.3e} > allowed {float(allowed.max()):.3e} (restatement {e:.3e})")
    rows = len(ref_pos)
    pos_tol = np.array([tol_p[r, ref_pos[r]] if ref_pos[r] >= 0 else 0.0 for r in range(rows)])
    decided = (margin == 0) | (margin > 2 * pos_tol)
    exempt = int((~decided).sum())
    got_pos = np.asarray(got_pos, np.int64)
    bad = decided & (got_pos != ref_pos)
    if bad.any():
        failures.append(f"positions differ at rows {np.argwhere(bad).ravel().tolist()}: got {got_pos[bad]}, reference {ref_pos[bad]} "
                        f"(margins {margin[bad]})")
    # the reported probability is p at the reported position
    for r in range(rows):
        if decided[r] and not bad[r]:
            want = ref_prob[r]
            if abs(float(got_prob[r]) - want) > pos_tol[r] + (SR.FLOOR if ref_pos[r] < 0 else 0.0):
                failures.append(f"prob of row {r}: {float(got_prob[r])!r} against {want!r}")
    if kind == "planted" and exempt:
        failures.append(f"{exempt} exempt rows in a planted case")
    report["margin_min"] = float(margin.min())
    return report, failures, exempt, rows
