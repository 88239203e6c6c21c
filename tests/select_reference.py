"""Plain numpy references of token selection and the AlignAtt read-out (csrc/select.hip, csrc/align_body.h).

Two statements of the same three operations:
  * float64 (`logsoftmax_topk`, `token_prob`, `alignatt`): what the kernels are compared with;
  * float32 (`logsoftmax_topk_f32`, `token_prob_f32`, `alignatt_f32`): numpy float32 throughout, two-pass max / exp-sum /
    log.  Its distance from the float64 form on a case is the yardstick the GPU test sizes its tolerance with, nothing else.
No torch in here."""
import numpy as np

FLOOR = 2.0 ** -22          # value tolerance floor, relative to max(1, |reference|)
KERNEL_FACTOR = 4.0         # the kernel may be this many times the float32 restatement's error


def apply_adjustments(logits, adj):
    """adj = (rows, ids, deltas); row < 0 = every row.  The addition is float32, as the kernel stores it."""
    x = np.array(logits, dtype=np.float32, copy=True)
    if adj is None:
        return x
    rows, ids, deltas = adj
    with np.errstate(invalid="ignore"):
        for r, i, d in zip(rows, ids, deltas):
            if r < 0:
                x[:, i] = x[:, i] + np.float32(d)
            else:
                x[r, i] = x[r, i] + np.float32(d)
    return x


def _order(x_row, k):
    """indices of the k best by (value descending, index ascending)"""
    return np.argsort(-x_row, kind="stable")[:k + 1]


def logsoftmax_topk(logits, adj, k):
    """-> (log-probabilities [R, k] float64, ids [R, k], gaps [R, k], adjusted float32 logits).
    gaps[r, j] = smallest log-probability distance from rank j to the ranks beside it (j - 1 and j + 1): 0 = an exact tie,
    which the index rule decides."""
    x32 = apply_adjustments(logits, adj)
    x = x32.astype(np.float64)
    R, V = x.shape
    vals = np.empty((R, k))
    ids = np.empty((R, k), np.int64)
    gaps = np.full((R, k), np.inf)
    with np.errstate(invalid="ignore", divide="ignore"):
        for r in range(R):
            mx = x[r].max()
            lp = (x[r] - mx) - np.log(np.exp(x[r] - mx).sum())
            o = _order(x[r], k)
            ids[r] = o[:k]
            vals[r] = lp[o[:k]]
            v = lp[o]
            d = np.abs(v[:-1] - v[1:])                      # rank j to rank j + 1 (nan for -inf beside -inf: a tie)
            d = np.where(np.isnan(d), 0.0, d)
            for j in range(k):
                if j < len(d):
                    gaps[r, j] = min(gaps[r, j], d[j])
                if j > 0:
                    gaps[r, j] = min(gaps[r, j], d[j - 1])
    return vals, ids, gaps, x32


def logsoftmax_topk_f32(logits, adj, k):
    x = apply_adjustments(logits, adj)
    R, V = x.shape
    vals = np.empty((R, k), np.float32)
    ids = np.empty((R, k), np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for r in range(R):
            mx = x[r].max()
            s = np.exp(x[r] - mx, dtype=np.float32).sum(dtype=np.float32)
            lse = np.log(s, dtype=np.float32)
            o = _order(x[r], k)[:k]
            ids[r] = o
            vals[r] = (x[r, o] - mx) - lse
    return vals, ids


def token_prob(logits, token):
    x = np.asarray(logits, np.float32).astype(np.float64)
    mx = x.max(axis=1, keepdims=True)
    e = np.exp(x - mx)
    return e[:, token] / e.sum(axis=1)


def token_prob_f32(logits, token):
    x = np.asarray(logits, np.float32)
    mx = x.max(axis=1, keepdims=True)
    e = np.exp(x - mx, dtype=np.float32)
    return (e[:, token] / e.sum(axis=1, dtype=np.float32)).astype(np.float32)


def window_rows(prefill_rows, n_single, single_base):
    """ring rows of the window in the order of row_of (align_body.h)"""
    return list(range(prefill_rows)) + [single_base + j for j in range(n_single)]


def median7_reflect(z):
    """width-7 median over the last axis with reflect padding; the identity when T <= 3 (whisper/timing.py:22-24)"""
    T = z.shape[-1]
    if T <= 3:
        return z
    idx = np.arange(-3, T + 3)
    idx = np.abs(idx)
    idx = np.where(idx >= T, 2 * (T - 1) - idx, idx)
    win = np.lib.stride_tricks.sliding_window_view(z[..., idx], 7, axis=-1)
    return np.sort(win, axis=-1)[..., 3]


def _alignatt(ring, counters, content_len, dt, zero_cols=()):
    ring = np.asarray(ring)
    A, B, _, T = ring.shape
    z = np.empty((B, A, T), dt)
    attn = np.empty((B, T), dt)
    frames = np.zeros(B, np.int64)
    margins = np.full(B, np.inf)
    eps = dt(1e-8)
    for b in range(B):
        pre, ns, newest, base = (int(c[b]) if np.ndim(c) else int(c) for c in counters)
        cl = int(content_len[b]) if np.ndim(content_len) else int(content_len)
        w = ring[:, b, window_rows(pre, ns, base), :].astype(dt)            # [A, n, T]
        mean = w.mean(axis=1, dtype=dt)
        std = np.sqrt(((w - mean[:, None, :]) ** 2).mean(axis=1, dtype=dt), dtype=dt)
        z[b] = (ring[:, b, newest, :].astype(dt) - mean) / (std + eps)
        z[b][:, list(zero_cols)] = 0
        attn[b] = median7_reflect(z[b]).mean(axis=0, dtype=dt)
        if cl > 0:
            cut = attn[b, :cl].astype(np.float64)
            f = int(np.argmax(cut))
            frames[b] = f
            if cl > 1:
                margins[b] = cut[f] - np.delete(cut, f).max()
    return z, attn, frames, margins


def alignatt(ring, counters, content_len):
    """ring [n_align][n_beam][ring_rows][T]; counters = (prefill_rows, n_single, newest_row, single_base), each a scalar or
    one entry per beam; content_len likewise.  -> (z [B, A, T], attn_last [B, T], frames [B], margins [B]): population
    mean / std per column over the window rows, z = (newest - mean) / (std + 1e-8), reflect-padded median of 7 over the
    full T, mean over the heads, first arg-max over [0, content_len) (frame 0 when that is empty); margin = winner minus the
    best other frame of that range (0 = exact tie, decided by the lowest frame)."""
    return _alignatt(ring, counters, content_len, np.float64)


def alignatt_f32(ring, counters, content_len, zero_cols=()):
    """zero_cols: columns that are constant over the window.  A float32 mean of n equal numbers need not be that number, so
    the restatement's 0 / 1e-8 there is noise of the order of 1e-3; such a column is no yardstick - z is required to be
    exactly 0 there (as the float64 form gives, and as a double accumulation gives) - and is set to 0 here."""
    return _alignatt(ring, counters, content_len, np.float32, zero_cols)


def value_tolerance(ref, f32):
    """-> (per-element allowed error, the restatement's own error): KERNEL_FACTOR x the float32 restatement's largest
    error on this case, floored at FLOOR * max(1, |reference|).  Equal infinities carry no error."""
    ref = np.asarray(ref, np.float64)
    e = abs_err(f32, ref)
    e32 = float(e.max()) if e.size else 0.0
    mag = np.where(np.isfinite(ref), np.abs(ref), 0.0)
    return np.maximum(KERNEL_FACTOR * e32, FLOOR * np.maximum(1.0, mag)), e32


def abs_err(got, ref):
    """|got - ref| with equal infinities (and nan beside nan) counting as 0 and unequal ones as inf"""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore"):
        e = np.abs(got - ref)
    same = (got == ref) | (np.isnan(got) & np.isnan(ref))
    e = np.where(same, 0.0, e)
    return np.where(np.isnan(e), np.inf, e)


# ----------------------------------------------------------------------------------------------------------------------
# a case (tests/select_cases.py) against these references
# ----------------------------------------------------------------------------------------------------------------------
def references(case):
    """both statements of everything a case asks for"""
    c = case
    counters = c["counters"]
    vals, ids, gaps, x32 = logsoftmax_topk(c["logits"], c["adj"], c["k"])
    vals32, ids32 = logsoftmax_topk_f32(c["logits"], c["adj"], c["k"])
    z, attn, frames, margins = alignatt(c["ring"], counters, c["content_len"])
    z32, attn32, frames32, _ = alignatt_f32(c["ring"], counters, c["content_len"], c["zero_cols"])
    ref = dict(top_vals=vals, top_ids=ids, gaps=gaps, logits_out=x32, z=z, attn_last=attn, frames=frames, margins=margins)
    f32 = dict(top_vals=vals32, top_ids=ids32, z=z32, attn_last=attn32, frames=frames32, logits_out=x32)
    if c["ns_token"] >= 0:
        ref["ns_probs"] = token_prob(c["ns_logits"], c["ns_token"])
        f32["ns_probs"] = token_prob_f32(c["ns_logits"], c["ns_token"])
    return ref, f32


def compare(case, ref, f32, got):
    """`got` (a kernel route's outputs, or the float32 restatement itself) against the float64 reference of `case`.
    -> (report, failures).  Values: within value_tolerance.  Integers: equal to the reference wherever its margin is an exact
    tie (0: the index rule decides) or exceeds twice the value tolerance; the pairs in between are excluded and counted -
    none allowed in planted / tie cases, at most 2 % in random ones."""
    report, failures = {}, []
    tols = {}
    for key in ("top_vals", "z", "attn_last", "ns_probs"):
        if key not in ref:
            continue
        allowed, e32 = value_tolerance(ref[key], f32[key])
        tols[key] = allowed
        err = abs_err(got[key], ref[key])
        worst = int(np.argmax(err - allowed)) if err.size else 0
        report[key] = dict(restatement_err=e32, kernel_err=float(err.max()), allowed=float(allowed.reshape(-1)[worst]))
        if (err > allowed).any():
            failures.append(f"{key}: error {err.reshape(-1)[worst]:.3e} > allowed {allowed.reshape(-1)[worst]:.3e} "
                            f"(restatement {e32:.3e}) at flat index {worst}")
    # ids
    gaps = ref["gaps"]
    decided = (gaps == 0) | (gaps > 2 * tols["top_vals"])
    n_excl = int((~decided).sum())
    bad = decided & (np.asarray(got["top_ids"]) != ref["top_ids"])
    if bad.any():
        failures.append(f"top_ids differ at (row, rank) {np.argwhere(bad).tolist()[:8]}: got {np.asarray(got['top_ids'])[bad][:8]}, "
                        f"reference {ref['top_ids'][bad][:8]}")
    # frames
    T = ref["attn_last"].shape[1]
    m = ref["margins"]
    frame_tol = np.array([tols["attn_last"][b, ref["frames"][b]] for b in range(len(m))])
    decided_f = (m == 0) | (m > 2 * frame_tol)
    n_excl_f = int((~decided_f).sum())
    bad = decided_f & (np.asarray(got["frames"]) != ref["frames"])
    if bad.any():
        failures.append(f"frames differ at rows {np.argwhere(bad).ravel().tolist()}: got {np.asarray(got['frames'])[bad]}, "
                        f"reference {ref['frames'][bad]} (margins {m[bad]})")
    cap = 0.02 if case["kind"] == "random" else 0.0
    report["excluded"] = dict(ids=n_excl, id_pairs=int(gaps.size), frames=n_excl_f, frame_rows=int(m.size))
    if n_excl > cap * gaps.size or n_excl_f > cap * m.size:
        failures.append(f"exclusions beyond the cap of a {case['kind']} case: {report['excluded']}")
    if not np.array_equal(np.asarray(got["logits_out"], np.float32).view(np.uint32), ref["logits_out"].view(np.uint32)):
        failures.append("the logits left in memory are not the float32-adjusted input")
    for col in case["zero_cols"]:
        if np.any(np.asarray(got["z"])[:, :, col] != 0):
            failures.append(f"z of the constant column {col} is not 0")
    return report, failures
