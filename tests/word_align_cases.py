"""Inputs of the word-alignment tests: one generator module for test_word_align_reference_cpu.py (which checks the references
on these very cases) and test_gpu_word_align.py (which runs them through wlk_diag_word_align).  Seeded by name.

A case: P token rows = [n_sot sot tokens, notimestamps, n_text text tokens, eot], F frames of T, n_align heads, raw scores
ring [n_align][ring_rows][T] with NaN in every column at or beyond F and every ring row at or beyond P, logits [n_text][ld]
with +1e30 in the columns at or beyond n_cols, targets [n_text], qk_scale.  nan_cols: (head, frame) pairs whose weights are
bit-identical in all rows (raw score -inf in every row: the weight is 0 in either number type), so z is 0 / 0 there."""
import functools

import numpy as np

from dec_attention_cases import hash_name

MAX_HEADS = None        # the largest head count of dims.ALIGNMENT_HEADS (set below)


def _max_heads():
    from whisperlivekit_amd.dims import ALIGNMENT_HEADS
    return max(len(v) for v in ALIGNMENT_HEADS.values())


MAX_HEADS = _max_heads()


def _rng(name):
    return np.random.default_rng(hash_name(name))


def make(name, P, F, n_align=1, n_sot=1, n_cols=7, ld=None, T=None, ring_rows=None, qk_scale=1.0, style="random",
         target="random", logit_spread=4.0, nan_cols=(), family="chain"):
    rng = _rng(name)
    n_text = P - n_sot - 2
    assert n_text >= 1
    ld = n_cols if ld is None else ld
    T = F + 5 if T is None else T
    ring_rows = P + 2 if ring_rows is None else ring_rows
    ring = np.full((n_align, ring_rows, T), np.nan, np.float32)
    if style == "uniform":          # columns nearly constant over the rows: std / mean about 1e-4
        x = rng.standard_normal((n_align, 1, F)) * 2 + 1e-4 * rng.standard_normal((n_align, P, F))
    else:
        x = rng.standard_normal((n_align, P, F)) * 3
    if style == "offset":
        x = x + 300
    if style == "ties":             # a frame repeats its left neighbour in every row: equal z in one window, bit for bit
        for f in range(1, F, 3):
            x[:, :, f] = x[:, :, f - 1]
        if F >= 6:
            x[:, :, 4] = x[:, :, 5] = x[:, :, 3]
    for a, f in nan_cols:
        x[a, :, f] = -np.inf
    ring[:, :P, :F] = x
    logits = np.full((n_text, ld), 1e30, np.float32)
    logits[:, :n_cols] = rng.standard_normal((n_text, n_cols)) * logit_spread
    if target == "first":
        targets = np.zeros(n_text, np.int32)
    elif target == "last":
        targets = np.full(n_text, n_cols - 1, np.int32)
    else:
        targets = rng.integers(0, n_cols, n_text).astype(np.int32)
    return dict(name=name, family=family, P=P, F=F, T=T, ring_rows=ring_rows, n_align=n_align, n_sot=n_sot, n_cols=n_cols, ld=ld,
                qk_scale=float(qk_scale), n_text=n_text, ring=ring, logits=logits, targets=targets, nan_cols=tuple(nan_cols))


def _specs():
    s = {}

    def add(name, **kw):
        assert name not in s
        s[name] = kw

    # token probability: n_cols around the 256-thread stride and at the vocabularies' eot, ld = n_cols and larger, targets
    # at both ends, 1 / 2 / 445 rows, a row spread over +-80
    for i, n_cols in enumerate((1, 2, 255, 256, 257, 50256, 51864)):
        rows = 445 if n_cols == 257 else 1 + i % 2
        add(f"prob_c{n_cols}", family="prob", P=3 + rows, F=4, n_cols=n_cols, ld=n_cols + (0, 3, 8)[i % 3],
            target=("first", "last", "random")[i % 3])
    add("prob_c257_first_padded", family="prob", P=5, F=4, n_cols=257, ld=300, target="first")
    add("prob_c256_last", family="prob", P=5, F=4, n_cols=256, ld=256, target="last")
    add("prob_spread80", family="prob", P=5, F=4, n_cols=51864, ld=51865, logit_spread=40.0)
    # softmax: T = 1500, F around the 256-thread stride, both scales, scores offset by +300
    for F in (1, 2, 3, 4, 255, 256, 257, 750, 1500):
        add(f"softmax_f{F}", family="softmax", P=5, F=F, T=1500, n_align=2, qk_scale=(1.0, 0.5)[F % 2])
    add("softmax_f257_half", family="softmax", P=5, F=257, T=1500, n_align=2, qk_scale=0.5)
    add("softmax_f256_offset300", family="softmax", P=5, F=256, T=1500, n_align=2, style="offset")
    add("softmax_f750_offset300_half", family="softmax", P=6, F=750, T=1500, n_align=1, style="offset", qk_scale=0.5)
    # z-score: P around the four row groups, F around the 64-frame workgroup, 1 / 3 / the most heads, nearly uniform columns
    for P, F, A in ((4, 1, 1), (5, 63, 3), (7, 64, 1), (8, 65, 3), (9, 1500, 3), (448, 65, 1), (5, 129, MAX_HEADS), (448, 129, 3)):
        add(f"zscore_p{P}_f{F}_a{A}", family="zscore", P=P, F=F, n_align=A)
    for P, F in ((4, 64), (9, 129), (448, 63)):
        add(f"zscore_uniform_p{P}_f{F}", family="zscore", P=P, F=F, n_align=3, style="uniform")
    # cost: F around the median padding and the 256-thread stride, n_sot 1 / 3 / 4, one and 444 text tokens, planted ties
    for i, F in enumerate((1, 2, 3, 4, 5, 6, 7, 8, 255, 256, 257)):
        n_sot = (1, 3, 4)[i % 3]
        add(f"cost_f{F}_sot{n_sot}", family="cost", P=n_sot + 3 + i % 2, F=F, n_align=2, n_sot=n_sot)
    add("cost_one_text_token_sot3", family="cost", P=6, F=9, n_align=3, n_sot=3)
    add("cost_444_text_tokens", family="cost", P=448, F=8, n_align=2, n_sot=2, T=16, ring_rows=448)
    add("cost_444_text_tokens_f257", family="cost", P=448, F=257, n_align=1, n_sot=2, ring_rows=448)
    for F in (4, 7, 30):
        add(f"cost_ties_f{F}", family="cost", P=8, F=F, n_align=2, n_sot=3, style="ties")
    # a NaN column: P = 4, one frame, then three adjacent frames (inside, and where the reflection doubles them)
    add("nan_one_frame", family="nan", P=4, F=12, n_align=2, nan_cols=((0, 5),))
    add("nan_three_frames", family="nan", P=4, F=14, n_align=2, nan_cols=((0, 6), (0, 7), (0, 8), (1, 7)))
    add("nan_three_frames_at_the_edge", family="nan", P=4, F=12, n_align=1, nan_cols=((0, 1), (0, 2), (0, 3)))
    add("nan_f5_both_reflections", family="nan", P=4, F=5, n_align=1, nan_cols=((0, 2),))
    # the whole chain, multilingual sot sequence
    add("chain_p6_f5_a1", family="chain", P=6, F=5, n_align=1, n_sot=3, n_cols=300, ld=301)
    add("chain_p40_f129_a3", family="chain", P=40, F=129, n_align=3, n_sot=3, n_cols=1000, ld=1000, T=1500, qk_scale=0.5)
    add("chain_p448_f1500_a10", family="chain", P=448, F=1500, n_align=10, n_sot=3, n_cols=257, ld=260, T=1500, ring_rows=448)
    return s


SPECS = _specs()
NAMES = tuple(SPECS)
BIG = ("chain_p448_f1500_a10",)


@functools.lru_cache(maxsize=4)
def case(name):
    return make(name, **SPECS[name])


def family(fam):
    return [n for n in NAMES if SPECS[n]["family"] == fam]
