"""The linear layers of csrc/gemm_f32.hip - the single-row and the staged GEMV kernel in every instantiation launch_gemv
reaches, and the GEMM kernels' epilogue operands (scale_period, the prefill's cache append, operand tables) - one operator
per call through wlk_diag_linear_ex (production launchers, unchanged), against the float64 reference of
tests/linear_reference.py on the cases of tests/linear_cases.py.  No model, no session, no graph.

Tolerance (tests/select_reference.py: value_tolerance): a value may be off by 4 x the error the float32 restatement has on
the same case (floor 2^-22 * max(1, |reference|)); the GEMV kernels' fused LayerNorm has a measured factor of its own
(linear_reference.OUTPUT_FACTOR).  Every buffer has guard words - a NaN bit pattern - behind it, the rows
of c are n + 4 apart and c and the caches arrive filled with the pattern: what the reference does not write must still hold
it, every input must come back bit for bit, what goes to a cache is bit for bit what goes to c, a launch repeated gives the
same bits, and on route 1 every row of a call is bit for bit that row sent alone.  Every case writes its errors to
linear_report.json in the directory WLK_REPORT_DIR names (default: test_reports/)."""
import json
import os

import numpy as np
import pytest

import linear_cases as LC
import linear_reference as LR
from linear_harness import WLK_ERR_ARG, Call, bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}


def report(key, value):
    REPORT[key] = value
    out = os.environ.get("WLK_REPORT_DIR") or os.path.join(ROOT, "test_reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "linear_report.json"), "w") as fh:
        json.dump(REPORT, fh, indent=1, sort_keys=True)


REFS = {}


def refs(c):
    """the float64 reference and the float32 restatement of a case, computed once"""
    if c["name"] not in REFS:
        REFS.clear()                    # (one case at a time: the largest is 2 x 8 x 32771 doubles)
        REFS[c["name"]] = (LR.linear(c, np.float64), LR.linear(c, np.float32))
    return REFS[c["name"]]


@pytest.mark.parametrize("name", LC.NAMES)
def test_linear(name):
    c = LC.case(name)
    ref, f32 = refs(c)
    failures, rep = [], {}
    for route in c["routes"]:
        tag = f"route{route}"
        first = Call(c, route)
        if first.rc != 0:
            failures.append(f"{tag}: error {first.rc}: {first.msg}")
            continue
        failures += first.check_words()
        entry, fail = LR.judge(tag, first.out, ref, f32, LC.family(c, route))
        rep[tag] = entry
        print(name, tag, json.dumps(entry))
        if fail:
            failures.append(fail)
        again = Call(c, route)
        if again.rc != 0 or not np.array_equal(bits(again.cbuf), bits(first.cbuf)) or (
                first.kc is not None and not (np.array_equal(bits(again.kc), bits(first.kc)) and
                                              np.array_equal(bits(again.vc), bits(first.vc)))):
            failures.append(f"{tag}: the same launch again gives other bits (rc {again.rc})")
        if route == 1 and (c["m"] > 1 or c["kv_mode"] == 2):
            # rows are independent and the single-row kernel is bit-identical to the staged one (csrc/gemm_f32.hip)
            for z in range(max(c["batch"], 1)):
                for row in range(c["m"]):
                    one = Call(LC.alone(c, z, row), 1)
                    if one.rc != 0:
                        failures.append(f"{tag}: row {row} alone: error {one.rc}: {one.msg}")
                    elif not np.array_equal(bits(one.out[0, 0]), bits(first.out[z, row])):
                        diff = bits(one.out[0, 0]) != bits(first.out[z, row])
                        failures.append(f"{tag}: row {row} differs from the same row alone in {int(diff.sum())} of {c['n']} features")
    report(name, rep)
    assert len(rep) == len(c["routes"]) and not failures, "\n".join(failures)


@pytest.mark.parametrize("what", list(LC.REFUSALS))
def test_refusals(what):
    base, override, route, fragment = LC.REFUSALS[what]
    call = Call(LC.case(base), override.get("route", route), **{k: v for k, v in override.items() if k != "route"})
    assert call.rc == WLK_ERR_ARG and fragment in call.msg, (what, call.rc, call.msg)
    assert not call.changed(["a", "w", "bias", "gamma", "beta", "r", "c", "kc", "vc"]), "a refused call touched a buffer"


def test_route_0_is_launch_linears_choice():
    """launch_linear by shape: the GEMV kernels up to 8 rows, the GEMM kernels from 9 on (512 x 120 x 256: the k-wave kernel) -
    the bits of the forced routes"""
    for name, forced in (("st_m8_n131_k2048", 1), ("gemm_period_kpipe", 2)):
        c = LC.case(name)
        a, b = Call(c, 0), Call(c, forced)
        assert a.rc == 0 and b.rc == 0, (a.msg, b.msg)
        assert np.array_equal(bits(a.cbuf), bits(b.cbuf)), name
