"""tests/linear_reference.py and tests/linear_cases.py without a GPU: the float64 reference against torch's linear /
layer_norm / gelu / silu in double on every case; the float32 restatement against the tolerance it defines; the case table
against launch_gemv's own dispatch (wlk_diag_gemv_variant: every instantiation the dispatch can reach has a case); and
every deliberate mistake of the reference module against that tolerance - a table that could not tell a mistake from the
reference would not test it."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import linear_cases as LC
import linear_reference as LR
from whisperlivekit_amd import _lib

WLK_ERR_ARG = -1


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).double()


def torch_linear(c):
    a = t64(c["a"])
    if c["gamma"] is not None:
        a = F.layer_norm(a, (c["k"],), t64(c["gamma"]), t64(c["beta"]), 1e-5)
    y = F.linear(a, t64(c["w"]), t64(c["bias"]) if c["bias"] is not None else None)
    if c["flags"] & LR.SCALE:
        col = torch.arange(c["n"])
        if c["scale_period"]:
            col = col % c["scale_period"]
        y = torch.where(col < c["scale_cols"], y * float(np.float32(c["scale"])), y)
    if c["flags"] & LR.GELU:
        y = F.gelu(y)
    if c["flags"] & LR.RELU:
        y = F.relu(y)
    if c["flags"] & LR.SWISH:
        y = F.silu(y)
    if c["flags"] & LR.RESIDUAL:
        y = y + t64(c["r"])
    return y.numpy()


@pytest.mark.parametrize("name", LC.NAMES)
def test_reference_is_torch_in_double_and_the_restatement_passes_its_own_rule(name):
    c = LC.case(name)
    ref, f32 = LR.linear(c, np.float64), LR.linear(c, np.float32)
    assert ref.dtype == np.float64 and f32.dtype == np.float32 and ref.shape == (max(c["batch"], 1), c["m"], c["n"])
    assert np.all(np.isfinite(ref))
    assert np.abs(ref - torch_linear(c)).max() <= 1e-11 * max(1.0, np.abs(ref).max())
    assert set(LR.OUTPUT_FACTOR) <= {"gemv_ln"} and {LC.family(c, r) for r in c["routes"]} <= {"gemv", "gemv_ln", "gemm"}
    entry, fail = LR.judge("restatement", f32, ref, f32)
    assert fail is None and np.isfinite(entry["restatement_err"]), (entry, fail)
    if c["kv_mode"]:
        idx = LR.cache_indices(c)
        assert idx.shape == (c["m"], c["kv_d"]) and idx.min() >= 0 and idx.max() < c["cache_floats"]
        assert len(np.unique(idx)) == idx.size, "two rows of a case append to the same cache words"
        if c["kv_mode"] == 1:                       # neither the first nor the last position of a beam's cache
            assert 0 < c["kv_pos"] and c["kv_pos"] + c["kv_ntok"] < c["kv_ctx"]
    # the inputs the table promises
    assert not c["w"][c["n"] // 2].any()


def test_the_table_holds_the_inputs_it_promises():
    kinds = {k for s in LC.SPECS.values() if s["ln"] for k in s["rows"]}
    assert kinds == set(LC.ROW_KINDS)
    c = LC.case("row_swish_minus100")
    pre = LR.linear(dict(c, flags=0), np.float64)
    assert pre.min() == -100.0 and np.sort(pre.reshape(-1))[1] > -9.0 and pre.max() > 7.0
    c = LC.case("row_big_residual")
    prod = LR.linear(dict(c, flags=0), np.float64)
    assert np.median(np.abs(c["r"])) > 500 * np.median(np.abs(prod))
    c = LC.case("row_const_ln")
    assert np.ptp(c["a"]) == 0.0
    flags = [s["flags"] for s in LC.SPECS.values() if s["routes"] == (1,) and s["m"] == 1]
    for bit in (LR.GELU, LR.RELU, LR.SWISH, LR.RESIDUAL, LR.SCALE):
        assert any(f & bit for f in flags)
    assert any(s["r_is_c"] for s in LC.SPECS.values() if s["m"] == 1)
    assert any(not s["bias"] for s in LC.SPECS.values()) and any(s["bias"] for s in LC.SPECS.values())


# ----------------------------------------------------------------------------------------------------------------------
def variant(m, n, k, ln, kv_mode, buf=C.create_string_buffer(200)):
    rc = _lib.load().wlk_diag_gemv_variant(m, n, k, int(ln), kv_mode, buf, len(buf))
    assert rc in (0, WLK_ERR_ARG)
    return rc, buf.value.decode()


def test_gemv_variant_names_what_the_kernel_comments_state():
    assert variant(1, 1280, 1280, True, 0) == (0, "gemv1<5,1,ln,full>")
    assert variant(1, 1152, 384, True, 1) == (0, "gemv1<2,1,ln,part>")
    assert variant(1, 5120, 1280, True, 0) == (0, "gemv1<5,2,ln,full>")
    assert variant(1, 1280, 5120, False, 0) == (0, "gemv1<20,1,plain,full>")
    assert variant(4, 2048, 512, False, 0) == (0, "gemv<4,2>")
    assert variant(1, 51864, 512, True, 0) == (0, "gemv<1,4>")
    assert variant(1, 1152, 384, True, 2) == (0, "gemv<1,1>")
    for args, fragment in (((9, 131, 128, False, 0), "unsupported shape"), ((1, 131, 6, False, 0), "unsupported shape"),
                           ((4, 131, 4100, False, 0), "unsupported shape"), ((0, 131, 128, False, 0), "m >= 1")):
        rc, text = variant(*args)
        assert rc == WLK_ERR_ARG and fragment in text, (args, rc, text)


def test_every_instantiation_the_dispatch_reaches_has_a_case():
    """the answers of launch_gemv's dispatch over the table = its answers over every shape class it accepts"""
    table = {}
    for name, s in LC.SPECS.items():
        if 1 in s["routes"]:
            rc, text = variant(s["m"], s["n"], s["k"], s["ln"], s["kv_mode"])
            assert rc == 0, (name, text)
            table.setdefault(text, name)
    sweep = set()
    ks = list(range(4, 5124 + 1, 4)) + [8192, 16384]
    for m in range(1, 9):
        for n in (131, 2049, 16385):
            for ln in (False, True):
                for kv_mode in (0, 1, 2):
                    for k in ks:
                        rc, text = variant(m, n, k, ln, kv_mode)
                        if rc == 0:
                            sweep.add(text)
    assert not any("mg" in v for v in sweep)
    missing, extra = sorted(sweep - set(table)), sorted(set(table) - sweep)
    assert not missing and not extra, f"instantiations without a case: {missing}; answers outside the sweep: {extra}"
    assert len(sweep) == 48 + 6 + 12        # UB 2 .. 8 x RPW x LN x FULL, UB 12 / 16 / 20 x FULL, MR x RPW


# ----------------------------------------------------------------------------------------------------------------------
def caught(mutated, ref, allowed):
    err = LR.abs_err(mutated, ref)
    return bool((err > allowed).any())


@pytest.mark.parametrize("mutant", LR.MUTANTS)
def test_the_cases_are_sharp(mutant):
    """at least one named case is further from the reference, under the mistake, than a kernel may be"""
    cache_mutant = mutant in ("append_pos1", "append_ntok1", "steprow_row0")
    applies = [n for n in LC.NAMES if mutant in LC.mutants(dict(LC.SPECS[n], bias=True if LC.SPECS[n]["bias"] else None))]
    assert applies, f"no case exercises {mutant}"
    catching = []
    for name in applies:
        c = LC.case(name)
        ref, f32 = LR.linear(c, np.float64), LR.linear(c, np.float32)
        if cache_mutant:
            for which in (0, 1):
                r_img, f_img = LR.cache_images(c, ref, np.nan)[which], LR.cache_images(c, f32, np.nan)[which]
                m_img = LR.cache_images(c, ref, np.nan, mutant)[which]
                grow = np.full(m_img.size - r_img.size, np.nan)           # a mistake may write behind the caches
                r_img, f_img = np.concatenate([r_img, grow]), np.concatenate([f_img, grow.astype(np.float32)])
                if caught(m_img, r_img, LR.value_tolerance(r_img, f_img)[0]):
                    catching.append(name)
                    break
        elif caught(LR.linear(c, np.float64, mutant), ref,      # (under the widest factor any route of the case is judged with)
                    max((LR.allowed_error(ref, f32, LC.family(c, r))[0] for r in c["routes"]), key=lambda a: a.max())):
            catching.append(name)
        if len(catching) >= 3:
            break
    assert catching, f"{mutant}: none of {applies} tells it from the reference"
