"""The contract of wlk_pick_topk (csrc/select.hip: rules_topk_kernel) stated in float64 numpy (TEST infrastructure only).

Per row, over the logits of the last decode step:
  allowed(v)   what wlk_pick_params describes (include/wlk_hip.h): not suppressed (mask bit 0), not a blank at the first step
               (bit 1), and - with timestamps - not <|notimestamps|>, not a timestamp behind a closed pair (ts_mode 1), not a
               text token behind an opening timestamp (ts_mode 2), not a timestamp below ts_bound, and at the first step a
               timestamp no later than max_initial.
  decision     if logsumexp(allowed timestamps) > max(allowed text) the text tokens drop out (decoding.py:487-499).
  result       the k best of what is left by (value descending, index ascending), as log_softmax over what is left;
               (-inf, -1) where fewer than k entries are left.

`near_ties` says where float64 itself is too close to call: the only places a float32 implementation may answer differently."""
import numpy as np

NEAR_TIE = 1e-4


def rules_mask(n_vocab, suppressed, blank):
    """The byte mask wlk_rules_set uploads: bit 0 = always suppressed, bit 1 = blank."""
    m = np.zeros(n_vocab, np.uint8)
    m[list(suppressed)] |= 1
    m[list(blank)] |= 2
    return m


def allowed(mask, st, n_vocab):
    v = np.arange(n_vocab)
    ok = (mask & 1) == 0
    if st["first_step"]:
        ok &= (mask & 2) == 0
    if st["without_timestamps"]:
        return ok
    tb = st["timestamp_begin"]
    if st["no_timestamps"] >= 0:
        ok[st["no_timestamps"]] = False
    if st["ts_mode"] == 1:
        ok &= v < tb
    if st["ts_mode"] == 2:
        ok &= v >= st["eot"]
    ok &= ~((v >= tb) & (v < st["ts_bound"]))
    if st["first_step"]:
        ok &= v >= tb
        if st["max_initial"] >= 0:
            ok &= v < tb + st["max_initial"] + 1
    return ok


def _logsumexp(x):
    m = x.max() if x.size else -np.inf
    if not np.isfinite(m):
        return -np.inf
    return m + np.log(np.exp(x - m).sum())


def _row(logits, mask, st, k):
    """-> (log-probabilities [k], ids [k], margin of the timestamps-versus-text decision, sorted values of the k + 1 best)."""
    V = logits.shape[0]
    x = np.where(allowed(mask, st, V), logits.astype(np.float64), -np.inf)
    tb = st["timestamp_begin"]
    norm = _logsumexp(x)
    margin = np.inf
    if not st["without_timestamps"]:
        lse_ts = _logsumexp(x[tb:])
        text = x[:tb].max() if tb > 0 else -np.inf
        if np.isfinite(lse_ts):
            if np.isfinite(text):
                margin = abs(lse_ts - text)
            if lse_ts > text:
                x[:tb] = -np.inf
                norm = lse_ts
    order = np.lexsort((np.arange(V), -x))[:k + 1]          # value descending, index ascending
    vals = x[order]
    lp = np.full(k, -np.inf)
    ids = np.full(k, -1, np.int32)
    n = min(k, int(np.isfinite(vals[:k]).sum()))
    lp[:n] = vals[:n] - norm
    ids[:n] = order[:n]
    return lp, ids, margin, vals


def rules_topk_reference(logits, mask, states, k):
    """logits [rows, n_vocab], mask [n_vocab] uint8, one wlk_pick_params dictionary per row -> (log-probabilities
    [rows, k] float64, ids [rows, k] int32)."""
    rows = [_row(np.asarray(logits[r]), mask, states[r], k) for r in range(len(states))]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def near_ties(logits, mask, states, k, eps=NEAR_TIE):
    """[rows, k] bool: entries where float64 is within `eps` of a tie - between this candidate and a neighbour in the
    ranking (the k + 1st included), or, for the whole row, in the timestamps-versus-text decision."""
    out = np.zeros((len(states), k), bool)
    for r in range(len(states)):
        _, _, margin, vals = _row(np.asarray(logits[r]), mask, states[r], k)
        if margin <= eps:
            out[r] = True
            continue
        with np.errstate(invalid="ignore"):
            gap = np.abs(np.diff(vals))                      # gap[i] between ranks i and i + 1 (nan between two -inf)
        close = np.nan_to_num(gap, nan=np.inf) <= eps
        out[r, :len(close)] |= close[:k]
        out[r, 1:] |= close[:k - 1]
    return out
