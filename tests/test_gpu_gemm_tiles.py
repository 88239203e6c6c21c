"""The tiled fp32 GEMM kernels of csrc/gemm_f32.hip, instantiation by instantiation: gemm_nt_f32_kernel<64,64> / <32,64>,
the k-wave kernels in their launch_gemm and their kp forms, and every one of the k-pipe kernel's eight tiles - one launch
per call through wlk_diag_linear_ex (production launchers, unchanged; route 500 + 10 tm + tn is launch_gemm_kp's tile
probe), against the float64 reference of tests/linear_reference.py on the cases of tests/gemm_tile_cases.py.  No model, no
session, no graph.  Which kernel a (case, route) reaches is asserted without a GPU (tests/test_gemm_tile_cases_cpu.py).

Tolerance (tests/select_reference.py: value_tolerance, per element): a value may be off by 4 x the error the float32
restatement has on the same case, floored at 2^-22 * max(1, |reference|); no kernel family here has a factor of its own.
Buffers are those of tests/linear_harness.py: guard words behind every operand set, between the rows of a where lda > k,
in the pad columns of c and r; c arrives filled with the pattern.  What the reference does not write must still hold it,
every input must come back bit for bit and a launch repeated gives the same bits.  Across launches: all eight k-pipe tiles
agree bit for bit, route 4 and route 5 with the tile their plan names; the first 300 rows of the 900-row case under every
tile are the 300-row case under the kp family's 16 x 16 and 32 x 32 k-wave forms; route 5 is the forced route
wlk_diag_gemm_plan names for it, route 0 likewise; operand set z of a table is that set sent alone.  Every case writes its
errors, and every kernel family its worst error / allowed, to gemm_tiles_report.json in the directory WLK_REPORT_DIR names
(default: test_reports/)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import gemm_tile_cases as GC
import linear_reference as LR
from linear_harness import WLK_ERR_ARG, Call, bits
from whisperlivekit_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {"cases": {}, "worst_of_allowed": {}}
CALLS = {}                              # (case, route) -> the outputs of the first launch, for the tests across launches


def report(name, rep, c):
    REPORT["cases"][name] = rep
    for tag, entry in rep.items():
        fam = GC.family(c, int(tag[5:]))
        worst = REPORT["worst_of_allowed"].setdefault(fam, dict(of_allowed=0.0, case=None))
        if entry["of_allowed"] >= worst["of_allowed"]:
            worst.update(of_allowed=entry["of_allowed"], case=f"{name} {tag}")
    out = os.environ.get("WLK_REPORT_DIR") or os.path.join(ROOT, "test_reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "gemm_tiles_report.json"), "w") as fh:
        json.dump(REPORT, fh, indent=1, sort_keys=True)


def plan(c, route, buf=C.create_string_buffer(256)):
    rc = _lib.load().wlk_diag_gemm_plan(c["m"], c["n"], c["k"], route, c["batch"], int(c["kv_mode"] != 0), buf, len(buf))
    assert rc == 0, (c["name"], route, buf.value.decode())
    return buf.value.decode()


def outputs(name, route, c=None):
    """the outputs [Z][m][n] of route `route` on case `name`: from test_tiles' launch, or launched now"""
    if (name, route) not in CALLS:
        call = Call(c if c is not None else GC.case(name), route)
        assert call.rc == 0, (name, route, call.msg)
        CALLS[name, route] = call.out.copy()
    return CALLS[name, route]


@pytest.mark.parametrize("name", GC.NAMES)
def test_tiles(name):
    c = GC.case(name)
    ref, f32 = LR.linear(c, np.float64), LR.linear(c, np.float32)
    failures, rep = [], {}
    for route in c["routes"]:
        tag = f"route{route}"
        first = Call(c, route)
        if first.rc != 0:
            failures.append(f"{tag}: error {first.rc}: {first.msg}")
            continue
        CALLS[name, route] = first.out.copy()
        failures += first.check_words()
        entry, fail = LR.judge(tag, first.out, ref, f32, GC.family(c, route))
        rep[tag] = entry
        print(name, tag, GC.PLAN[name][route], json.dumps(entry))
        if fail:
            failures.append(fail)
        again = Call(c, route)
        if again.rc != 0 or not np.array_equal(bits(again.cbuf), bits(first.cbuf)):
            failures.append(f"{tag}: the same launch again gives other bits (rc {again.rc})")
    # across the routes of the case: any tile gives the same bits, and a launcher's own choice (routes 0 and 5; route 4 beside
    # the tile probes) is bit for bit the forced route of the kernel wlk_diag_gemm_plan names for it
    tiles = [r for r in c["routes"] if r in GC.TILE_ROUTES]
    pairs = [(tiles[0], r) for r in tiles[1:]]
    for own in (0, 5) + ((4,) if tiles else ()):
        if own in c["routes"]:
            kernel = plan(c, own)
            twins = [r for r in c["routes"] if r not in (0, 5, own) and GC.PLAN[name][r] == kernel]
            if twins:
                pairs.append((own, max(twins)))
    pairs = [p for p in pairs if (name, p[0]) in CALLS and (name, p[1]) in CALLS]           # (a failed launch is reported above)
    for pair in pairs:
        a, b = (CALLS[name, r] for r in pair)
        if not np.array_equal(bits(a), bits(b)):
            failures.append(f"route {pair[0]} and route {pair[1]} differ in {int((bits(a) != bits(b)).sum())} of {a.size} outputs")
    if c["batch"]:                  # an operand set of a table is that set alone
        for route in c["routes"]:
            for z in range(c["batch"]):
                one = Call(GC.set_alone(c, z), route)
                if one.rc != 0:
                    failures.append(f"route {route}: set {z} alone: error {one.rc}: {one.msg}")
                elif (name, route) in CALLS and not np.array_equal(bits(one.out[0]), bits(CALLS[name, route][z])):
                    failures.append(f"route {route}: set {z} of the table differs from the same set alone")
    report(name, rep, c)
    assert len(rep) == len(c["routes"]) and not failures, "\n".join(failures)


@pytest.mark.parametrize("name", list(GC.HEAD_OF))
def test_rows_keep_their_bits_whatever_is_stacked_under_them(name):
    """the kp family's promise: the first rows of the parent under every k-pipe tile are the head case under the 16 x 16
    and both 32 x 32 k-wave forms"""
    parent, rows = GC.HEAD_OF[name]
    head = GC.case(name)
    differing = []
    for hr in head["routes"]:
        h = outputs(name, hr, head)
        for pr in GC.TILE_ROUTES:
            p = outputs(parent, pr)
            if not np.array_equal(bits(p[:, :rows]), bits(h)):
                differing.append((pr, hr, int((bits(p[:, :rows]) != bits(h)).sum())))
    assert not differing, f"(tile route, k-wave route, differing outputs): {differing}"


@pytest.mark.parametrize("what", list(GC.REFUSALS))
def test_refusals(what):
    base, route, fragment = GC.REFUSALS[what]
    call = Call(GC.case(base), route)
    assert call.rc == WLK_ERR_ARG and fragment in call.msg, (what, call.rc, call.msg)
    assert not call.changed(["a", "w", "bias", "gamma", "beta", "r", "c", "kc", "vc"]), "a refused call touched a buffer"
