"""tests/word_align_reference.py against torch double forms of the reference's own lines (whisper/timing.py:197-214 as
oracle/timing_oracle.alignment_cost restates them: softmax, std_mean(unbiased=False), whisper_oracle.median_filter, the
slice and the head mean), on the cases the GPU test runs; every deliberate mistake must be told from the reference by some
named case at the GPU test's own tolerance; the NaN order of the median is kept on record."""
import functools

import numpy as np
import pytest
import torch

import word_align_cases as WC
import word_align_reference as WR
from oracle import timing_oracle, whisper_oracle

SMALL = [n for n in WC.NAMES if n not in WC.BIG]
TORCH_CASES = ["prob_c257", "prob_c51864", "prob_spread80", "softmax_f3", "softmax_f257_half", "softmax_f256_offset300",
               "zscore_p4_f1_a1", "zscore_p8_f65_a3", "zscore_uniform_p9_f129", "cost_f4_sot1", "cost_f7_sot1", "cost_ties_f7",
               "cost_one_text_token_sot3", "nan_three_frames", "nan_three_frames_at_the_edge", "chain_p40_f129_a3"]


@functools.lru_cache(maxsize=None)
def both(name):
    c = WC.case(name)
    return WR.chain(c), WR.chain(c, np.float32)


def same(a, b, rtol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b))
    np.testing.assert_allclose(np.nan_to_num(a), np.nan_to_num(b), rtol=rtol, atol=0)


def test_the_case_list_covers_what_it_names():
    assert set(TORCH_CASES) <= set(WC.NAMES)
    assert WC.MAX_HEADS == 23 and "zscore_p5_f129_a23" in WC.NAMES
    for name in WC.NAMES:
        c = WC.case(name) if name not in WC.BIG else None
        if c is None:
            continue
        assert np.isnan(c["ring"][:, c["P"]:, :]).all() and np.isnan(c["ring"][:, :, c["F"]:]).all()
        assert not np.isnan(c["ring"][:, :c["P"], :c["F"]]).any()
        assert (c["logits"][:, c["n_cols"]:] == np.float32(1e30)).all()
        assert c["targets"].min() >= 0 and c["targets"].max() < c["n_cols"]


@pytest.mark.parametrize("name", TORCH_CASES)
def test_float64_statement_is_the_references_arithmetic(name):
    c = WC.case(name)
    ref, _ = both(name)
    P, F, n_sot = c["P"], c["F"], c["n_sot"]
    with torch.no_grad():
        logits = torch.from_numpy(c["logits"]).double()
        probs = logits[:, :c["n_cols"]].softmax(dim=-1)[np.arange(c["n_text"]), list(c["targets"])]
        raw = torch.from_numpy(c["ring"]).double()
        w = (raw[:, :P, :F] * c["qk_scale"]).softmax(dim=-1)
        std, mean = torch.std_mean(w, dim=-2, keepdim=True, unbiased=False)
        z = (w - mean) / std
        m = whisper_oracle.median_filter(z, 7)
        cost = -(m.mean(dim=0)[n_sot:-1])
    same(ref["probs"], probs.numpy(), 1e-12)
    same(ref["w"], w.numpy(), 1e-12)
    same(ref["z"], z.numpy(), 1e-7)          # (torch's std is a one-pass form: the uniform columns differ in the 9th digit)
    assert np.array_equal(WR.median7(z.numpy()), m.numpy(), equal_nan=True)
    same(WR.cost_from_z(z.numpy(), n_sot), cost.numpy(), 1e-12)
    same(ref["cost"], cost.numpy(), 1e-6)
    assert ref["cost"].shape == (c["n_text"] + 1, F)


@pytest.mark.parametrize("name", ["cost_f8_sot3", "cost_ties_f30", "chain_p40_f129_a3"])
def test_float32_statement_is_close_and_passes_its_own_tolerance(name):
    ref, f32 = both(name)
    for key in ref:
        assert f32[key].dtype == np.float32
    _, failures = WR.compare(ref, f32, f32)
    assert not failures
    assert float(np.abs(f32["cost"] - ref["cost"]).max()) < 1e-4


@pytest.mark.parametrize("mistake", WR.MISTAKES)
def test_some_case_rejects_the_mistake(mistake):
    for name in SMALL:
        ref, f32 = both(name)
        with np.errstate(all="ignore"):
            wrong = WR.chain(WC.case(name), np.float64, mistake)
        if WR.compare(ref, f32, wrong)[1]:
            return
    pytest.fail(f"no case of word_align_cases.py tells '{mistake}' from the reference: a case is missing")


@pytest.mark.parametrize("name", WC.family("nan"))
def test_nan_columns_and_the_order_of_the_median(name):
    """z is NaN exactly in the planted columns; the median orders a NaN last, as torch.sort does; the fminf / fmaxf network
    wa_median7 used to be drops it instead - the two disagree on every one of these cases"""
    c = WC.case(name)
    for dt in (np.float64, np.float32):
        r = WR.chain(c, dt)
        planted = np.zeros((c["n_align"], c["F"]), bool)
        for a, f in c["nan_cols"]:
            planted[a, f] = True
        assert np.array_equal(np.isnan(r["z"]), np.broadcast_to(planted[:, None, :], r["z"].shape))
        with torch.no_grad():
            want = whisper_oracle.median_filter(torch.from_numpy(r["z"]), 7).numpy()
        assert np.array_equal(WR.median7(r["z"]), want, equal_nan=True)
        old = WR.median7_dropping_nan(r["z"])
        assert not np.array_equal(old, want, equal_nan=True)
        finite = ~np.isnan(r["z"]).any(axis=(1, 2))
        assert np.array_equal(WR.median7_dropping_nan(r["z"][finite]), WR.median7(r["z"][finite]))
    ref = WR.chain(c)
    trace = timing_oracle.dtw_trace(ref["cost"].astype(np.float32))
    assert trace.shape == (c["n_text"] + 2, c["F"] + 1) and (trace[0] == -1).all() and (trace[:, 0] == -1).all()


def test_the_old_network_agrees_with_the_sort_on_finite_windows():
    z = np.random.default_rng(7).standard_normal((3, 5, 40)).astype(np.float32)
    z[:, :, 10] = z[:, :, 11]
    assert np.array_equal(WR.median7_dropping_nan(z), WR.median7(z))
