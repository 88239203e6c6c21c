"""Token selection and the AlignAtt read-out (csrc/select.hip, csrc/align_body.h) on chosen inputs, through
wlk_diag_select: every route that accepts a case against the float64 reference of tests/select_reference.py, and the
routes against each other bit for bit.  No model, no session.

Tolerances (tests/select_reference.py: value_tolerance / compare): a value may be off by 4 x the error the float32
restatement has on the same case (floor 2^-22 * max(1, |reference|)); ids and frames equal the reference wherever its
margin is an exact tie or exceeds twice that tolerance.  Every case writes both errors and its exclusions to
select_report.json in the directory WLK_REPORT_DIR names (default: test_reports/ in the repository root)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import select_cases as SC
import select_reference as SR
from whisperlivekit_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}
WLK_ERR_ARG = -1


def report(key, value):
    REPORT[key] = value
    out = os.environ.get("WLK_REPORT_DIR") or os.path.join(ROOT, "test_reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "select_report.json"), "w") as fh:
        json.dump(REPORT, fh, indent=1, sort_keys=True)


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def run_route(case, route):
    """-> (rc, outputs or the error text)"""
    lib = _lib.load()
    logits = np.ascontiguousarray(case["logits"], np.float32)
    R, V = logits.shape
    ring = np.ascontiguousarray(case["ring"], np.float32)
    A, B, ring_rows, T = ring.shape
    assert B == R
    k = case["k"]
    pre, ns, newest, base = case["counters"]
    keep = [logits, ring]
    q = _lib.DiagSelectArgs()
    q.route, q.n_rows, q.n_vocab, q.k = route, R, V, k
    q.logits = vp(logits)
    if case["adj"] is not None:
        rows, ids, deltas = (np.ascontiguousarray(a, t) for a, t in zip(case["adj"], (np.int32, np.int32, np.float32)))
        keep += [rows, ids, deltas]
        q.adj_row, q.adj_ids, q.adj_deltas, q.n_adj = vp(rows), vp(ids), vp(deltas), len(ids)
    q.n_align, q.ring_rows, q.T, q.single_base = A, ring_rows, T, int(base)
    q.ring = vp(ring)
    counters = [np.ascontiguousarray(a, np.int32) for a in (pre, ns, newest, case["content_len"])]
    keep += counters
    q.prefill_rows, q.n_single, q.newest_row, q.content_len = (vp(a) for a in counters)
    q.ns_token = int(case["ns_token"])
    if case["ns_token"] >= 0:
        nsl = np.ascontiguousarray(case["ns_logits"], np.float32)
        keep.append(nsl)
        q.ns_logits = vp(nsl)
    out = dict(top_vals=np.full((R, k), np.nan, np.float32), top_ids=np.full((R, k), -1, np.int32),
               frames=np.full(R, -1, np.int32), attn_last=np.full((R, T), np.nan, np.float32),
               z=np.full((R, A, T), np.nan, np.float32), ns_probs=np.full(R, np.nan, np.float32),
               logits_out=np.full((R, V), np.nan, np.float32))
    q.top_logprobs, q.top_ids, q.frames, q.attn_last = vp(out["top_vals"]), vp(out["top_ids"]), vp(out["frames"]), vp(out["attn_last"])
    q.z, q.ns_probs, q.logits_out = vp(out["z"]), vp(out["ns_probs"]), vp(out["logits_out"])
    rc = lib.wlk_diag_select(C.byref(q))
    if rc != 0:
        return rc, lib.wlk_diag_last_error().decode()
    return 0, out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def check_case(name):
    case = SC.build(name)
    ref, f32 = SR.references(case)
    want = SC.expected_routes(case)
    outs, failures, rep = {}, [], {}
    for route in range(5):
        rc, out = run_route(case, route)
        if route not in want:
            if rc != WLK_ERR_ARG:
                failures.append(f"route {route} must refuse this case with WLK_ERR_ARG, answered {rc}")
            continue
        if rc != 0:
            failures.append(f"route {route}: error {rc}: {out}")
            continue
        outs[route] = out
        r, f = SR.compare(case, ref, f32, out)
        rep[f"route{route}"] = r
        print(name, "route", route, json.dumps(r))
        failures += [f"route {route}: {m}" for m in f]
    first = min(outs) if outs else None
    keys = ["top_vals", "top_ids", "frames", "attn_last", "z", "logits_out"] + (["ns_probs"] if case["ns_token"] >= 0 else [])
    for route, out in outs.items():
        for key in keys:
            if not np.array_equal(bits(out[key]), bits(outs[first][key])):
                n = int((bits(out[key]) != bits(outs[first][key])).sum())
                failures.append(f"route {route} and route {first} differ in {n} elements of {key}")
    rep["routes"] = sorted(outs)
    report(name, rep)
    assert sorted(outs) == want and not failures, "\n".join(failures)


@pytest.mark.parametrize("name", SC.TOPK_NAMES)
def test_topk(name):
    check_case(name)


@pytest.mark.parametrize("name", SC.ALIGN_NAMES)
def test_alignatt(name):
    check_case(name)


def test_unrunnable_shapes_are_refused_not_rerouted():
    case = SC.build("win_11_5_a30b1_peakT4")               # 30 heads x 1500 frames: beyond the LDS forms
    for route in (2, 3):
        rc, msg = run_route(case, route)
        assert rc == WLK_ERR_ARG and "fused" in msg, (route, rc, msg)
    case = SC.build("nospeech_v51864")
    rc, msg = run_route(case, 3)
    assert rc == WLK_ERR_ARG and "no-speech" in msg, (rc, msg)
    case = SC.build("rows4")
    for route in (0, 1, 2, 3):
        rc, msg = run_route(case, route)
        assert rc == WLK_ERR_ARG and "one set" in msg, (route, rc, msg)
    case = SC.build("T7")
    case["counters"] = (case["counters"][0], case["counters"][1], np.array([10 ** 6], np.int32), case["counters"][3])
    rc, msg = run_route(case, 0)
    assert rc == WLK_ERR_ARG and "leave the ring" in msg, (rc, msg)
