"""tests/cross_ragged_reference.py against a torch double form of the same attention, on the cases the GPU test runs; every
deliberate mistake must be told from the reference by some named case at the GPU test's own tolerance."""
import functools

import numpy as np
import pytest
import torch

import cross_ragged_cases as RC
import cross_ragged_reference as RR

TORCH_CASES = ["alone_t1", "alone_t129", "alone_t512", "mixed_g1", "mixed_g3_shuffled", "mixed_h16", "offset300", "peak60",
               "no_head_kept"]


@functools.lru_cache(maxsize=None)
def both(name):
    c = RC.case(name)
    return RR.attention(c), RR.attention(c, np.float32)


def test_the_case_list_covers_what_the_kernel_can_get_wrong():
    assert set(TORCH_CASES) <= set(RC.NAMES)
    alone = sorted(int(RC.SPECS[n]["lengths"][0]) for n in RC.NAMES if n.startswith("alone_t") and "_h16" not in n)
    assert tuple(alone) == RC.LENGTHS
    mixed = [n for n in RC.NAMES if n.startswith("mixed_g")]
    assert len(mixed) == 8 and all(len(RC.SPECS[n]["lengths"]) == 8 for n in mixed)
    assert {RC.SPECS[n].get("H", 2) for n in RC.NAMES} == {1, 2, 16}
    assert {(RC.SPECS[n].get("L", 1), RC.SPECS[n].get("layer", 0)) for n in RC.NAMES} >= {(1, 0), (3, 0), (3, 2)}
    for name in RC.NAMES:
        c = RC.case(name)
        for r, b in enumerate(c["blocks"]):
            T, lo, hi = int(c["lengths"][r]), c["kv_off"], c["kv_off"] + 2 * c["d"]
            assert np.isnan(b[T:]).all() and np.isnan(b[:, :lo]).all() and np.isnan(b[:, hi:]).all()
            assert not np.isnan(b[:T, lo:hi]).any()
        rank = c["head_rank"]
        assert sorted(rank[rank >= 0]) == list(range(c["n_rank"])) or (rank < 0).all()
    assert any((RC.case(n)["head_rank"] < 0).any() and (np.diff(RC.case(n)["head_rank"][RC.case(n)["head_rank"] >= 0]) < 0).any()
               for n in RC.NAMES), "no rank table with -1 entries and permuted ranks"


@pytest.mark.parametrize("name", TORCH_CASES)
def test_float64_statement_is_softmax_attention(name):
    c = RC.case(name)
    ref, f32 = both(name)
    d, H = c["d"], c["H"]
    for r in range(c["n_rows"]):
        T = int(c["lengths"][r])
        kv = torch.from_numpy(c["blocks"][r][:T, c["kv_off"]:c["kv_off"] + 2 * d]).double()
        q = torch.from_numpy(c["q"][r]).double().view(H, 1, 64)
        k = kv[:, :d].reshape(T, H, 64).permute(1, 0, 2)
        v = kv[:, d:].reshape(T, H, 64).permute(1, 0, 2)
        p = (q @ k.transpose(1, 2)).softmax(dim=-1)
        np.testing.assert_allclose(ref["out"][r], (p @ v).reshape(d).numpy(), rtol=1e-9, atol=1e-12)
        for h in range(H):
            if c["head_rank"][h] >= 0:
                got = ref["probs"][c["head_rank"][h], r]
                np.testing.assert_allclose(got[:T], p[h, 0].numpy(), rtol=1e-9, atol=1e-300)
                assert np.isnan(got[T:]).all()
    assert np.isnan(ref["probs"][:, c["n_rows"]:]).all()
    np.testing.assert_allclose(ref["sums"], 1.0, rtol=1e-12)
    assert not RR.compare(ref, f32, f32)[1]


def test_a_key_60_above_the_rest_gives_its_value_row():
    c = RC.case("peak60")
    ref, f32 = both("peak60")
    d = c["d"]
    want = np.empty_like(ref["out"])
    for r in range(c["n_rows"]):
        for h in range(c["H"]):
            sl = slice(h * 64, (h + 1) * 64)
            want[r, sl] = c["blocks"][r][c["peak"][r, h], c["kv_off"] + d:c["kv_off"] + 2 * d][sl]
    assert not RR.compare(dict(out=ref["out"]), dict(out=f32["out"]), dict(out=want))[1]


@pytest.mark.parametrize("mistake", RR.MISTAKES)
def test_some_case_rejects_the_mistake(mistake):
    for name in RC.NAMES:
        ref, f32 = both(name)
        with np.errstate(all="ignore"):
            wrong = RR.attention(RC.case(name), np.float64, mistake)
        if RR.compare(ref, f32, wrong)[1]:
            return
    pytest.fail(f"no case of cross_ragged_cases.py tells '{mistake}' from the reference: a case is missing")
