"""Plain numpy references of the decoder's attention stage (csrc/decoder.hip, the merged out projection of
csrc/gemm_f32.hip, the prefill flash kernel of csrc/attention.hip), for the routes of wlk_diag_dec_attention.

Two statements of every floating-point operation, from the same float32 inputs:
  * float64 (`dt=np.float64`): what the kernels are compared with;
  * float32 (`dt=np.float32`): numpy float32 throughout (dot products, max, exp, sum, division, weighted sum).  Its
    distance from the float64 form on a case is the yardstick the GPU test sizes its tolerance with, nothing else.
The ancestry update, the cache gather and the cache appends are exact: integer and copy models.  No torch in here.

Tolerance (select_reference.value_tolerance, unchanged): a value may be off by KERNEL_FACTOR x the restatement's largest
error on the same case and output, floored at FLOOR * max(1, |reference|)."""
import numpy as np

from select_reference import FLOOR, KERNEL_FACTOR, abs_err, value_tolerance  # noqa: F401  (the rule lives there)

HEAD = 64
# Factor of KERNEL_FACTOR-times-restatement that an output may use instead, keyed by output name.  Empty: no route has
# needed one.  An entry may only be added beside the MI355X measurement that shows summation order to be the cause
# (worst measured ratio x 1.5), never from a route's output on the case it judges.
OUTPUT_FACTOR = {}


def _softmax(s, dt):
    mx = s.max(axis=-1, keepdims=True)
    e = np.exp((s - mx).astype(dt), dtype=dt)
    return (e / e.sum(axis=-1, keepdims=True, dtype=dt)).astype(dt)


def _dot_rows(K, q, dt):
    """K [n, 64] . q [64] -> [n]"""
    return (K.astype(dt) * q.astype(dt)[None, :]).sum(axis=1, dtype=dt)


def _weighted(p, V, dt):
    """sum_j p[j] V[j, :]"""
    return (p.astype(dt)[:, None] * V.astype(dt)).sum(axis=0, dtype=dt)


# ----------------------------------------------------------------------------------------------------------------------
# self-attention over the cache
# ----------------------------------------------------------------------------------------------------------------------
def self_attention(qkv, kc, vc, n_tok, offsets, n_head, dt=np.float64, row_cache=None, anc=None):
    """qkv [n_rows * n_tok][3 d]; kc / vc [cache rows][ctx_len][d].  Query row r = b * n_tok + p sees positions
    [0, offset_b + p + 1) of its hypothesis.  Position j of hypothesis b lies in cache row
      row_cache[b]                   (rows form; offsets has one entry per row),
      min(anc[b][j], n_rows - 1)     (ancestry form),
      b                              otherwise.
    -> out [n_rows * n_tok][d]"""
    qkv = np.asarray(qkv, np.float32)
    QR, d = qkv.shape[0], qkv.shape[1] // 3
    n_rows = QR // n_tok
    offsets = np.atleast_1d(offsets)
    out = np.zeros((QR, d), dt)
    for r in range(QR):
        b, p = divmod(r, n_tok)
        off = int(offsets[b] if len(offsets) > 1 else offsets[0])
        n_keys = off + p + 1
        j = np.arange(n_keys)
        if anc is not None:
            src = np.minimum(np.asarray(anc)[b, :n_keys].astype(np.int64), n_rows - 1)
        elif row_cache is not None:
            src = np.full(n_keys, int(row_cache[b]))
        else:
            src = np.full(n_keys, b)
        for h in range(n_head):
            sl = slice(h * HEAD, (h + 1) * HEAD)
            s = _dot_rows(kc[src, j, sl], qkv[r, sl], dt)
            out[r, sl] = _weighted(_softmax(s, dt), vc[src, j, sl], dt)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# cross-attention
# ----------------------------------------------------------------------------------------------------------------------
def layernorm(x, gamma, beta, dt):
    x = np.asarray(x, np.float32).astype(dt)
    mean = x.mean(axis=-1, keepdims=True, dtype=dt)
    var = ((x - mean) ** 2).mean(axis=-1, keepdims=True, dtype=dt)
    return ((x - mean) / np.sqrt(var + dt(1e-5), dtype=dt) * gamma.astype(dt) + beta.astype(dt)).astype(dt)


def folded_query(x, wq, bq, gamma, beta, scale, dt=np.float64):
    """q = scale * (Wq . LN(x) + b): the bias is added before the scale"""
    h = layernorm(x, gamma, beta, dt)
    q = h @ np.asarray(wq, np.float32).astype(dt).T
    if bq is not None:
        q = q + np.asarray(bq, np.float32).astype(dt)
    return (q * dt(scale)).astype(dt)


def cross_attention(q, k, v, n_head, dt=np.float64, row_kv=None):
    """q [R][d] (any float type: the folded form hands its own precision on), k / v [n_kv][T][d]; row r uses set row_kv[r]
    (0 without).  -> (out [R][d], probabilities [R][H][T] over ALL T keys, raw scores [R][H][T])"""
    q = np.asarray(q)
    R, d = q.shape
    T = k.shape[1]
    out = np.zeros((R, d), dt)
    probs = np.zeros((R, n_head, T), dt)
    scores = np.zeros((R, n_head, T), dt)
    for r in range(R):
        s_ = 0 if row_kv is None else int(row_kv[r])
        for h in range(n_head):
            sl = slice(h * HEAD, (h + 1) * HEAD)
            s = _dot_rows(k[s_, :, sl], q[r, sl], dt)
            p = _softmax(s, dt)
            scores[r, h], probs[r, h] = s, p
            out[r, sl] = _weighted(p, v[s_, :, sl], dt)
    return out, probs, scores


def out_projection(att, wo, bo, resid, dt=np.float64):
    """resid + bo + Wo . att, one row"""
    y = np.asarray(wo, np.float32).astype(dt) @ att.astype(dt)
    return ((y + np.asarray(bo, np.float32).astype(dt)) + np.asarray(resid, np.float32).astype(dt)).astype(dt)


def cross_reference(case, route, dt):
    """what `route` must leave for a cross-attention case: dict(out, scores, align {(rank, beam, ring_row): row})"""
    c = case
    if route == "C2":
        q = folded_query(c["x"], c["wq"], c["bq"], c["gamma"], c["beta"], c["scale"], dt)
    else:
        q = np.asarray(c["q"], np.float32)
    att, probs, scores = cross_attention(q, c["k"], c["v"], c["H"], dt, c["row_kv"] if route == "C4" else None)
    res = dict(out=att, scores=scores, align={})
    if route == "C3":
        res["out"] = out_projection(att[0], c["wo"], c["bo"], c["resid"], dt)[None, :]
    if c["head_rank"] is not None:
        for r in range(c["R"]):
            for h, rank in enumerate(c["head_rank"]):
                if rank >= 0:
                    res["align"][(int(rank), int(c["beam_of_row"][r]), int(c["ring_row"][r]))] = probs[r, h]
    return res


# ----------------------------------------------------------------------------------------------------------------------
# exact models
# ----------------------------------------------------------------------------------------------------------------------
def anc_update(anc, ctl, offset, n_rows):
    """one launch_anc_update on anc [rows >= n_rows][ctx_len] uint8; ctl = (src 0..6, fresh).  Hypothesis b continues
    hypothesis ctl[b]: it inherits that row's columns below `offset`; from `offset` on it is in its own physical row."""
    anc = np.array(anc, np.uint8, copy=True)
    ctx_len = anc.shape[1]
    old = np.tile(np.arange(n_rows, dtype=np.int64)[:, None], (1, ctx_len)) if ctl[7] != 0 else anc[:n_rows].astype(np.int64)
    for b in range(n_rows):
        row = np.full(ctx_len, b, np.int64)
        sb = int(ctl[b])
        if 0 <= sb < n_rows:
            row[:max(0, min(int(offset), ctx_len))] = old[sb, :max(0, min(int(offset), ctx_len))]
        anc[b] = np.minimum(row, n_rows - 1).astype(np.uint8)
    return anc


def kv_gather(src, source_rows, length):
    """src [L][n_rows][ctx_len][d] -> (dst positions [0, length) of every row; the rest is not written)"""
    return src[:, np.asarray(source_rows), :length, :]


def kv_append(kc, vc, qkv, n_tok, offsets, row_cache=None):
    """k | v of every qkv row into kc / vc [rows][ctx_len][d] (copies returned)"""
    kc, vc = np.array(kc, copy=True), np.array(vc, copy=True)
    d = qkv.shape[1] // 3
    offsets = np.atleast_1d(offsets)
    for r in range(qkv.shape[0]):
        b, p = divmod(r, n_tok)
        if row_cache is not None:
            row, pos = int(row_cache[b]), int(offsets[b])
        else:
            row, pos = b, int(offsets[0]) + p
        kc[row, pos] = qkv[r, d:2 * d]
        vc[row, pos] = qkv[r, 2 * d:]
    return kc, vc


# ----------------------------------------------------------------------------------------------------------------------
# comparison
# ----------------------------------------------------------------------------------------------------------------------
def judge(name, got, ref, f32):
    """-> (report entry, failure text or None) for one output of one route on one case"""
    allowed, e32 = value_tolerance(ref, f32)
    if name in OUTPUT_FACTOR:
        mag = np.where(np.isfinite(ref), np.abs(ref), 0.0)
        allowed = np.maximum(OUTPUT_FACTOR[name] * e32, FLOOR * np.maximum(1.0, mag))
    err = abs_err(got, ref)
    worst = int(np.argmax(err - allowed))
    entry = dict(kernel_err=float(err.max()), restatement_err=e32, allowed=float(allowed.reshape(-1)[worst]),
                 of_allowed=float((err / allowed).max()), x_restatement=float(err.max() / e32) if e32 > 0 else None)
    fail = None
    if not np.all(np.isfinite(np.asarray(got, np.float64))):
        fail = f"{name}: not finite"
    elif (err > allowed).any():
        fail = (f"{name}: error {err.reshape(-1)[worst]:.3e} > allowed {allowed.reshape(-1)[worst]:.3e} "
                f"(restatement {e32:.3e}) at flat index {worst}")
    return entry, fail
