"""The float64 references of tests/select_reference.py against independent statements of the same operations (torch
float64, the oracle's AlignAtt), their tie ordering, and - on every case test_gpu_select.py runs - the exclusion caps for
the float32 restatement alone.  No GPU."""
import numpy as np
import pytest
import torch

import select_cases as SC
import select_reference as SR
from oracle import whisper_oracle as wo


@pytest.mark.parametrize("name", SC.TOPK_NAMES)
def test_topk_reference_matches_torch_float64(name):
    c = SC.build(name)
    vals, ids, gaps, x32 = SR.logsoftmax_topk(c["logits"], c["adj"], c["k"])
    x = torch.from_numpy(c["logits"].copy())
    if c["adj"] is not None:
        for r, i, d in zip(*c["adj"]):
            if r < 0:
                x[:, i] += float(d)
            else:
                x[r, i] += float(d)
    assert np.array_equal(x.numpy().view(np.uint32), x32.view(np.uint32))
    tv, ti = torch.log_softmax(x.double(), -1).topk(c["k"], dim=-1)
    assert SR.abs_err(vals, tv.numpy()).max() < 1e-12
    untied = gaps > 0
    assert np.array_equal(ids[untied], ti.numpy()[untied])
    # stated order: value descending, index ascending
    for r in range(ids.shape[0]):
        pairs = [(-float(x32[r, i]), int(i)) for i in ids[r]]
        assert pairs == sorted(pairs)
        rest = np.delete(x32[r], ids[r])
        if rest.size:
            assert rest.max() <= x32[r, ids[r, -1]]
            if rest.max() == x32[r, ids[r, -1]]:                # a tie left outside: it has a higher index
                assert int(np.flatnonzero(x32[r] == rest.max()).max()) > int(ids[r, -1])
    if c["ns_token"] >= 0:
        p = torch.softmax(torch.from_numpy(c["ns_logits"]).double(), -1)[:, c["ns_token"]].numpy()
        assert np.abs(SR.token_prob(c["ns_logits"], c["ns_token"]) - p).max() < 1e-14


def test_tie_order_is_lowest_index_first():
    x = np.zeros((1, 1000), np.float32)
    x[0, [900, 3, 512, 77]] = 4.0
    x[0, 600] = 5.0
    vals, ids, gaps, _ = SR.logsoftmax_topk(x, None, 4)
    assert ids.tolist() == [[600, 3, 77, 512]]
    assert gaps[0, 0] > 0 and gaps[0, 2] == 0
    ring = np.zeros((1, 1, 3, 1500), np.float32)
    ring[0, 0] = np.tile(np.random.default_rng(0).random((3, 250)).astype(np.float32), (1, 6))
    z, attn, frames, margins = SR.alignatt(ring, (3, 0, 2, 3), 1500)
    best = np.flatnonzero(attn[0] == attn[0].max())
    assert frames[0] == best.min() and (len(best) == 1 or margins[0] == 0)


def _torch_alignatt(ring, counters, b):
    pre, ns, newest, base = (int(np.asarray(c).reshape(-1)[b]) if np.ndim(c) else int(c) for c in counters)
    rows = SR.window_rows(pre, ns, base)
    a = torch.from_numpy(ring[:, b, rows, :]).double().unsqueeze(0)               # [1, A, n, T]
    std, mean = torch.std_mean(a, dim=-2, keepdim=True, unbiased=False)
    a = (a - mean) / (std + 1e-8)
    z = a[0, :, rows.index(newest), :]
    med = wo.median_filter(a, 7)[0, :, rows.index(newest), :]
    return z.numpy(), med.mean(dim=0).numpy()


@pytest.mark.parametrize("name", SC.ALIGN_NAMES)
def test_alignatt_reference_matches_oracle_pieces(name):
    c = SC.build(name)
    z, attn, frames, margins = SR.alignatt(c["ring"], c["counters"], c["content_len"])
    assert np.isfinite(z).all() and np.isfinite(attn).all()
    for b in range(z.shape[0]):
        tz, ta = _torch_alignatt(c["ring"], c["counters"], b)
        assert np.abs(z[b] - tz).max() <= 1e-9 * max(1.0, np.abs(tz).max())
        assert np.abs(attn[b] - ta).max() <= 1e-9 * max(1.0, np.abs(ta).max())
        cl = int(c["content_len"][b])
        assert frames[b] == (int(np.argmax(attn[b, :cl])) if cl else 0)


def test_alignatt_reference_matches_oracle_end_to_end():
    """scores -> oracle.alignatt_attention (softmax inside) against the reference fed with the same softmax rows"""
    rng = np.random.default_rng(5)
    A, T, pre, ns = 3, 1500, 11, 5
    steps = [[torch.from_numpy(rng.standard_normal((1, A, pre if s == 0 else 1, T)))] for s in range(ns + 1)]
    got = wo.alignatt_attention(steps, [(0, h) for h in range(A)], 1, 1300, 1)[0, -1].numpy()
    base = pre + 2
    ring = np.zeros((A, 1, base + 16, T))
    ring[:, 0, :pre] = torch.softmax(steps[0][0], -1)[0].numpy()
    for s in range(ns):
        ring[:, 0, base + s] = torch.softmax(steps[s + 1][0], -1)[0, :, 0].numpy()
    z, attn, frames, _ = SR.alignatt(ring, (pre, ns, base + ns - 1, base), 1300)
    assert np.abs(attn[0, :1300] - got).max() < 1e-9
    assert frames[0] == int(got.argmax())


@pytest.mark.parametrize("name", SC.ALIGN_NAMES + SC.TOPK_NAMES)
def test_float32_restatement_stays_within_the_exclusion_caps(name):
    c = SC.build(name)
    ref, f32 = SR.references(c)
    report, failures = SR.compare(c, ref, f32, f32)
    assert not failures, failures
    for col in c["zero_cols"]:
        assert not ref["z"][:, :, col].any()
    assert sorted(set(SC.expected_routes(c))) == SC.expected_routes(c) and 4 in SC.expected_routes(c)
