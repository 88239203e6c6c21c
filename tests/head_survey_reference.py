"""References of the alignment-head survey kernel (csrc/head_survey.hip) on the cases of tests/head_survey_cases.py.

The float64 statement: scores s[l][h][p][f] = q[l][p][64 h:64 h + 64] . k[f][l 2 d + 64 h: + 64], softmax over [:F], the
peak of every row and the LOWEST position that attains the row maximum; denom = 1 / peak = sum_f exp(s_f - max s).
The float32 restatement: a plain k-ordered fp32 dot product (one rounded multiply and one rounded add per k) and a numpy
float32 softmax denominator.  Its error against the float64 statement is the yardstick of the GPU test
(select_reference.value_tolerance)."""
import numpy as np


def scores(c, dtype=np.float64):
    """[L, H, P, F] in `dtype`; float32: accumulated k by k in float32"""
    L, H, P, F, d = c["n_layer"], c["n_head"], c["P"], c["F"], 64 * c["n_head"]
    q = c["q"].reshape(L, P, H, 64).transpose(0, 2, 1, 3)                               # [L, H, P, 64]
    k = c["k"][:F].reshape(F, L, 2, H, 64)[:, :, 0].transpose(1, 2, 0, 3)               # [L, H, F, 64]
    if dtype == np.float64:
        return np.einsum("lhpk,lhfk->lhpf", q.astype(np.float64), k.astype(np.float64))
    s = np.zeros((L, H, P, F), np.float32)
    for j in range(64):
        s = s + q[:, :, :, None, j] * k[:, :, None, :, j]
    assert s.dtype == np.float32
    return s


def fold(s):
    """scores [..., F] -> (denom, peak, frame) in the scores' own number type; frame = lowest arg-max"""
    m = s.max(axis=-1, keepdims=True)
    denom = np.exp(s - m).sum(axis=-1, dtype=s.dtype)
    return denom, (1 / denom).astype(s.dtype), s.argmax(axis=-1).astype(np.int32)


def top_gap(s64, dups=()):
    """lead of every row's top score over the runner-up among DISTINCT keys (`dups`: positions that repeat an earlier
    key bit for bit)"""
    s = s64.copy()
    if len(dups):
        s[..., list(dups)] = -np.inf
    if s.shape[-1] == 1:
        return np.full(s.shape[:-1], np.inf)
    top2 = np.partition(s, -2, axis=-1)[..., -2:]
    return top2[..., 1] - top2[..., 0]


def reference(c):
    """-> dict(denom64, peak64, frame64, denom32, gap)"""
    s64 = scores(c)
    d64, p64, f64 = fold(s64)
    d32, _, _ = fold(scores(c, np.float32))
    return dict(denom64=d64, peak64=p64, frame64=f64, denom32=d32, gap=top_gap(s64, c["dups"]), smax=float(np.abs(s64).max()))
