"""The contract of wlk_pick_topk (csrc/select.hip: rules_topk_kernel) stated in float64 numpy (TEST infrastructure only).

Per row, over the logits of the last decode step:
  allowed(v)   what wlk_pick_params describes (include/wlk_hip.h): not suppressed (mask bit 0), not a blank at the first step
               (bit 1), and - with timestamps - not <|notimestamps|>, not a timestamp behind a closed pair (ts_mode 1), not a
               text token behind an opening timestamp (ts_mode 2), not a timestamp below ts_bound, and at the first step a
               timestamp no later than max_initial.
  decision     if logsumexp(allowed timestamps) > max(allowed text) the text tokens drop out (decoding.py:487-499).
  result       the k best of what is left by (value descending, index ascending), as log_softmax over what is left;
               (-inf, -1) where fewer than k entries are left.

`near_ties` says where float64 itself is too close to call: the only places a float32 implementation may answer differently.
`exact_ties` tells the ties the contract itself decides (gap 0: the lower id ranks first) from those.  `history_state` is
what ApplyTimestampRules.apply reads from a sampled history, as the fields of wlk_pick_params; `rules_topk_f32` restates the
contract in float32 numpy, to measure what float32 alone costs against float64 (tests/test_gpu_rules_pick.py)."""
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
    if V > k + 1:                                           # only what reaches the k + 1st largest value (ties with it included)
        cand = np.flatnonzero(x >= np.partition(x, V - (k + 1))[V - (k + 1)])
    else:
        cand = np.arange(V)
    order = cand[np.lexsort((cand, -x[cand]))][:k + 1]      # value descending, index ascending
    vals = x[order]
    if len(vals) < k + 1:                                   # a vocabulary of no more than k entries: the ranking ends in -inf
        vals = np.concatenate([vals, np.full(k + 1 - len(vals), -np.inf)])
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


def exact_ties(logits, mask, states, k):
    """[rows, k] bool: entries whose value is bit-equal to a neighbour's in the ranking (the k + 1st included).  Such a tie is
    no near-tie: float64 and float32 see the same two numbers, and the contract ranks the lower id first."""
    out = np.zeros((len(states), k), bool)
    for r in range(len(states)):
        _, _, _, vals = _row(np.asarray(logits[r]), mask, states[r], k)
        with np.errstate(invalid="ignore"):
            same = np.isfinite(vals[:-1]) & (np.diff(vals) == 0.0)
        out[r, :len(same)] |= same[:k]
        out[r, 1:] |= same[:k - 1]
    return out


def unplanted_near_ties(logits, mask, states, k, eps=NEAR_TIE):
    """[rows, k] bool: `near_ties` without the entries that are close to a neighbour ONLY because they equal it: a gap in
    (0, eps] to either neighbour, or a decision margin within eps, still counts."""
    out = np.zeros((len(states), k), bool)
    for r in range(len(states)):
        _, _, margin, vals = _row(np.asarray(logits[r]), mask, states[r], k)
        if margin <= eps:
            out[r] = True
            continue
        with np.errstate(invalid="ignore"):
            gap = np.nan_to_num(np.abs(np.diff(vals)), nan=np.inf)
        close = (gap <= eps) & (gap > 0.0)
        out[r, :len(close)] |= close[:k]
        out[r, 1:] |= close[:k - 1]
    return out


def history_state(history, tb, eot, no_timestamps, max_initial, without_timestamps):
    """The wlk_pick_params of the pick that follows the sampled tokens `history` (whisper/decoding.py:441-499 reads the whole
    history: the last token, the one before it, and the last timestamp anywhere in it)."""
    h = [int(t) for t in history]
    last_ts = len(h) >= 1 and h[-1] >= tb
    before_last_ts = len(h) < 2 or h[-2] >= tb
    stamps = [t for t in h if t >= tb]
    bound = tb
    if stamps:
        bound = stamps[-1] if (last_ts and not before_last_ts) else stamps[-1] + 1
    return dict(first_step=int(len(h) == 0), without_timestamps=int(bool(without_timestamps)), timestamp_begin=int(tb), eot=int(eot),
                no_timestamps=int(no_timestamps), ts_mode=0 if not last_ts else (1 if before_last_ts else 2), ts_bound=int(bound),
                max_initial=int(max_initial))


def rules_topk_f32(logits, mask, states, ids):
    """The contract in float32 numpy, evaluated at the float64 ranking `ids` [rows, k]: max, sum exp(x - max) and
    (x - max) - log(sum) in float32, the decision as logsumexp(timestamps) > max(text).  -> log-probabilities [rows, k]
    float32 (-inf where ids is -1).  Only a yardstick for the error float32 arithmetic has on a case."""
    f = np.float32
    out = np.full(np.shape(ids), -np.inf, f)
    for r in range(len(states)):
        st, row = states[r], np.asarray(logits[r], f)
        x = np.where(allowed(mask, st, row.shape[0]), row, f(-np.inf))
        tb = st["timestamp_begin"]

        def fold(v):
            m = v.max() if v.size else f(-np.inf)
            if not np.isfinite(m):
                return m, f(0)
            return m, np.exp(v - m, dtype=f).sum(dtype=f)
        m_all, s_all = fold(x)
        mx, logsum = m_all, np.log(s_all, dtype=f)
        if not st["without_timestamps"]:
            m_ts, s_ts = fold(x[tb:])
            text = x[:tb].max() if tb > 0 else f(-np.inf)
            if np.isfinite(m_ts) and f(m_ts + np.log(s_ts, dtype=f)) > text:
                mx, logsum = m_ts, np.log(s_ts, dtype=f)
        for j, v in enumerate(np.asarray(ids[r])):
            if v >= 0:
                out[r, j] = f(f(x[v] - mx) - logsum)
    return out
