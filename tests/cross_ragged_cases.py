"""Inputs of the ragged cross-attention tests: one generator module for test_cross_ragged_reference_cpu.py and
test_gpu_cross_ragged.py (wlk_diag_nllb_cross_ragged).  Seeded by name.

A case: n_rows rows of H heads (d = 64 H), row r with lengths[r] keys in a block of its own, blocks[r] [kv_rows[r]][ldkv],
ldkv = 2 d L with k | v of the layer in use at kv_off = 2 d layer; NaN in every key row at or beyond the row's length and in
the other layers' columns.  head_rank [H] (-1: not kept) with n_rank ranks, stride = the alignment rows' length.
style: "random"; "offset" (every score near +300); "peak" (one key - peak[r][h] - 60 above the rest)."""
import functools

import numpy as np

from dec_attention_cases import hash_name

HEAD = 64
LENGTHS = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 130, 143, 144, 145, 255, 256, 257, 383, 384, 385, 511, 512)
GROUPS = (LENGTHS[0:8], LENGTHS[8:16], LENGTHS[16:24], LENGTHS[24:26] + (129, 1, 257, 64, 385, 16))
SHUFFLE = (3, 7, 0, 5, 2, 6, 1, 4)


def _ranks(rng, H):
    """a rank table with -1 entries and permuted ranks (one head: kept)"""
    if H == 1:
        return np.array([0], np.int32), 1
    keep = np.sort(rng.choice(H, size=max(1, H // 2), replace=False))
    rank = np.full(H, -1, np.int32)
    rank[keep] = rng.permutation(len(keep))
    return rank, len(keep)


def make(name, lengths, H=2, L=1, layer=0, style="random", stride=None, ranks="mixed"):
    rng = np.random.default_rng(hash_name(name))
    lengths = np.asarray(lengths, np.int32)
    R, d = len(lengths), HEAD * H
    ldkv, kv_off = 2 * d * L, 2 * d * layer
    q = (rng.standard_normal((R, d)) * 0.35).astype(np.float32)
    blocks, kv_rows, peak = [], [], np.zeros((R, H), np.int64)
    for r in range(R):
        T = int(lengths[r])
        rows = T + 2
        b = np.full((rows, ldkv), np.nan, np.float32)
        k = rng.standard_normal((T, d)) * 0.35
        v = rng.standard_normal((T, d))
        if style != "random":           # key j of head h scores target[j] (up to rounding): k = target q / (q . q)
            for h in range(H):
                sl = slice(h * HEAD, (h + 1) * HEAD)
                qh = q[r, sl].astype(np.float64)
                target = rng.standard_normal(T)
                if style == "offset":
                    target = target + 300
                else:
                    peak[r, h] = rng.integers(0, T)
                    target[peak[r, h]] = target.max() + 60
                k[:, sl] = target[:, None] * qh[None, :] / (qh @ qh)
        b[:T, kv_off:kv_off + d] = k
        b[:T, kv_off + d:kv_off + 2 * d] = v
        blocks.append(b)
        kv_rows.append(rows)
    if ranks == "none":
        head_rank, n_rank = np.full(H, -1, np.int32), 1
    else:
        head_rank, n_rank = _ranks(rng, H)
    return dict(name=name, n_rows=R, H=H, d=d, L=L, layer=layer, kv_off=kv_off, ldkv=ldkv, lengths=lengths, kv_rows=kv_rows,
                blocks=blocks, q=q, head_rank=head_rank, n_rank=n_rank, stride=int(stride or max(lengths)), style=style, peak=peak)


def _specs():
    s = {}
    for i, T in enumerate(LENGTHS):             # every length alone
        L = (1, 3)[i % 2]
        s[f"alone_t{T}"] = dict(lengths=[T], H=(1, 2)[(i // 2) % 2], L=L, layer=(0, L - 1)[(i // 3) % 2],
                                stride=(None, 512)[i % 2])
    for g, group in enumerate(GROUPS):          # eight to a launch, in two orders
        s[f"mixed_g{g}"] = dict(lengths=list(group), H=2, L=3, layer=(0, 2)[g % 2], stride=512)
        s[f"mixed_g{g}_shuffled"] = dict(lengths=[group[i] for i in SHUFFLE], H=(1, 2)[g % 2], L=1, stride=None)
    s["mixed_h16"] = dict(lengths=[512, 129, 17, 1, 384, 145, 64, 257], H=16, L=1, stride=512)
    s["alone_t130_h16_l3"] = dict(lengths=[130], H=16, L=3, layer=2)
    s["offset300"] = dict(lengths=[5, 129, 512, 64], H=2, L=1, style="offset")
    s["offset300_h16"] = dict(lengths=[257, 3], H=16, L=1, style="offset")
    s["peak60"] = dict(lengths=[2, 17, 130, 512, 255, 128, 385, 65], H=2, L=3, layer=2, style="peak")
    s["no_head_kept"] = dict(lengths=[130, 7], H=2, L=1, ranks="none")
    return s


SPECS = _specs()
NAMES = tuple(SPECS)


@functools.lru_cache(maxsize=4)
def case(name):
    return make(name, **SPECS[name])


def alone(c, r):
    """row r of a case as a launch of its own (the same operands)"""
    out = dict(c)
    out.update(name=f"{c['name']}[{r}]", n_rows=1, lengths=c["lengths"][r:r + 1], kv_rows=c["kv_rows"][r:r + 1],
               blocks=c["blocks"][r:r + 1], q=c["q"][r:r + 1], peak=c["peak"][r:r + 1])
    return out
