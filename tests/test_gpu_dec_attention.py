"""The decoder's attention stage (csrc/decoder.hip, the merged out projection of csrc/gemm_f32.hip, the prefill flash
kernel of csrc/attention.hip) on chosen inputs, through wlk_diag_dec_attention: every route that takes a case against the
float64 reference of tests/dec_attention_reference.py, the routes that promise the same bits against each other, the
integer and copy kernels against exact models.  No model, no session.

Tolerance (tests/select_reference.py: value_tolerance): a value may be off by 4 x the error the float32 restatement has on
the same case and output (floor 2^-22 * max(1, |reference|)).  Every buffer a route writes is larger than what it may
write and arrives filled with a NaN bit pattern: whatever the route does not address must still hold it.  Every case
writes its errors to dec_attention_report.json in the directory WLK_REPORT_DIR names (default: test_reports/).

This file was written without access to a GPU and has not yet run on an MI355X: no error figure is recorded here."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import dec_attention_cases as DC
import dec_attention_reference as DR
from whisperlivekit_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}
WLK_ERR_ARG = -1
GUARD = np.uint32(0x7FC12345)           # a NaN with a payload: reading it poisons, and it is recognisable
ROUTE = dict(S0=_lib.DA_S0, S1=_lib.DA_S1, S2=_lib.DA_S2, C0=_lib.DA_C0, C1=_lib.DA_C1, C2=_lib.DA_C2, C3=_lib.DA_C3,
             C4=_lib.DA_C4, C5=_lib.DA_C5, A0=_lib.DA_A0, G0=_lib.DA_G0, K0=_lib.DA_K0, K1=_lib.DA_K1)


def report(key, value):
    REPORT[key] = value
    out = os.environ.get("WLK_REPORT_DIR") or os.path.join(ROOT, "test_reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "dec_attention_report.json"), "w") as fh:
        json.dump(REPORT, fh, indent=1, sort_keys=True)


def guard(shape):
    return np.full(shape, GUARD, np.uint32).view(np.float32)


def is_guard(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint32) == GUARD))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def call(route, **kw):
    """-> (rc, message).  Arrays are passed by pointer (in / out buffers are changed in place), numbers by value."""
    a = _lib.DiagDecAttentionArgs()
    a.route = ROUTE[route]
    keep = []
    for key, val in kw.items():
        if val is None:
            continue
        if isinstance(val, np.ndarray):
            assert val.flags["C_CONTIGUOUS"], key
            keep.append(val)
            setattr(a, key, val.ctypes.data_as(C.c_void_p))
        else:
            setattr(a, key, val)
    lib = _lib.load()
    rc = lib.wlk_diag_dec_attention(C.byref(a))
    return rc, ("" if rc == 0 else lib.wlk_diag_last_error().decode())


def i32(a):
    return np.ascontiguousarray(a, np.int32)


# ----------------------------------------------------------------------------------------------------------------------
# self-attention
# ----------------------------------------------------------------------------------------------------------------------
def run_self(case, route, anc=None):
    """-> (rc, message, out rows)"""
    c = case
    n_rows, n_tok, d, ctx_len = c["n_rows"], c["n_tok"], c["d"], c["ctx_len"]
    QR = n_rows * n_tok
    out = guard((QR + 3, d))
    kc, vc = c["kc"].copy(), c["vc"].copy()
    kw = dict(n_rows=n_rows, n_tok=n_tok, d=d, n_head=c["H"], ctx_len=ctx_len, qkv=c["qkv"], kcache=kc, vcache=vc,
              cache_floats=kc.size, out=out, out_floats=out.size)
    one = c["offsets"][:1]
    if route == "S0":
        kw["offsets"] = i32(one)
    elif route == "S1":
        rows_form = c["form"] == "rows"
        kw["offsets"] = i32(c["offsets"] if rows_form else np.repeat(one, n_rows))
        kw["row_cache"] = i32(c["row_cache"] if rows_form else np.arange(n_rows))
        kw["layer_off"] = c["layer_off"] or 1028
    else:
        table = anc if anc is not None else c["anc"]
        if table is None:
            table = np.tile(np.arange(n_rows, dtype=np.uint8)[:, None], (1, ctx_len))
        table = np.ascontiguousarray(table, np.uint8)
        kw.update(offsets=i32(one), anc=table, anc_rows=table.shape[0])
    rc, msg = call(route, **kw)
    if rc == 0:
        assert is_guard(out[QR:]), f"{route} wrote behind its {QR} output rows"
        assert np.array_equal(bits(kc), bits(c["kc"])) and np.array_equal(bits(vc), bits(c["vc"]))
    return rc, msg, out[:QR]


SELF_REF = {}


def self_refs(case):
    if case["name"] not in SELF_REF:
        kw = dict(row_cache=case["row_cache"] if case["form"] == "rows" else None, anc=case["anc"] if case["form"] == "anc" else None)
        args = (case["qkv"], case["kc"], case["vc"], case["n_tok"], case["offsets"], case["H"])
        SELF_REF[case["name"]] = (DR.self_attention(*args, np.float64, **kw), DR.self_attention(*args, np.float32, **kw))
    return SELF_REF[case["name"]]


@pytest.mark.parametrize("name", DC.SELF_NAMES)
def test_self_attention(name):
    case = DC.build(name)
    want = DC.expected_routes(case)
    failures, rep, outs = [], {}, {}
    for route, fragment in case["refused"].items():
        rc, msg, _ = run_self(case, route)
        if rc != WLK_ERR_ARG or fragment not in msg:
            failures.append(f"{route} must refuse with '{fragment}', answered {rc}: {msg}")
    if want:
        ref, f32 = self_refs(case)
    for route in want:
        rc, msg, out = run_self(case, route)
        if rc != 0:
            failures.append(f"{route}: error {rc}: {msg}")
            continue
        outs[route] = out
        entry, fail = DR.judge("out", out, ref, f32)
        rep[route] = dict(out=entry)
        print(name, route, json.dumps(entry))
        if fail:
            failures.append(f"{route}: {fail}")
    for route, out in outs.items():
        if not np.array_equal(bits(out), bits(outs[want[0]])):
            failures.append(f"{route} and {want[0]} differ in {int((bits(out) != bits(outs[want[0]])).sum())} elements")
    # a rewind leaves old rows behind the key count: they must not reach the output
    for fill in (np.nan, 1e30):
        poisoned = DC.stale(case, np.float32(fill))
        for route in outs:
            rc, msg, out = run_self(poisoned, route)
            if rc != 0 or not np.all(np.isfinite(out)) or not np.array_equal(bits(out), bits(outs[route])):
                failures.append(f"{route}: {fill} behind the key count changes the output (rc {rc} {msg})")
    if case["anc_alt"] is not None and "S2" in outs:
        rc, msg, out = run_self(case, "S2", anc=case["anc_alt"])
        if rc != 0 or not np.array_equal(bits(out), bits(outs["S2"])):
            failures.append(f"S2: the table that differs only where it must not matter changes the output (rc {rc} {msg})")
    rep["routes"] = sorted(outs)
    report(name, rep)
    assert sorted(outs) == sorted(want) and not failures, "\n".join(failures)


# ----------------------------------------------------------------------------------------------------------------------
# cross-attention
# ----------------------------------------------------------------------------------------------------------------------
def run_cross(case, route, k_splits=1, q=None):
    """-> (rc, message, dict(out, scores, ring))"""
    c = case
    R, d, H, T = c["R"], c["d"], c["H"], c["T"]
    out = guard((R + 2, d))
    scores = guard(R * H * T + 64)
    kw = dict(n_rows=R, n_tok=1, d=d, n_head=H, T=T, k=c["k"], v=c["v"], n_kv=c["n_kv"], k_splits=k_splits, out=out,
              out_floats=out.size, scores=scores, scores_floats=scores.size)
    if route == "C4":
        kw["row_kv"] = i32(c["row_kv"])
    else:
        kw.update(k=np.ascontiguousarray(c["k"][:1]), v=np.ascontiguousarray(c["v"][:1]), n_kv=1)
    if route == "C2":
        kw.update(x=c["x"], wq=c["wq"], bq=c["bq"], gamma=c["gamma"], beta=c["beta"], scale=c["scale"])
    else:
        kw["q"] = c["q"] if q is None else q
    if route == "C3":
        kw.update(wo=c["wo"], bo=c["bo"], resid=c["resid"])
    ring = None
    if c["head_rank"] is not None:
        ring = guard((c["n_align"], c["n_beam"], c["ring_rows"], T))
        kw.update(head_rank=i32(c["head_rank"]), n_align=c["n_align"], n_beam=c["n_beam"], ring_rows=c["ring_rows"],
                  ring_row=i32(c["ring_row"]), beam_of_row=i32(c["beam_of_row"]), ring=ring)
    rc, msg = call(route, **kw)
    n_out = 1 if route == "C3" else R
    if rc == 0:
        assert is_guard(out[n_out:]), f"{route} wrote behind its {n_out} output rows"
        assert is_guard(scores[R * H * T:]) and (route != "C5" or is_guard(scores)), f"{route} wrote outside its scores"
    return rc, msg, dict(out=out[:n_out], scores=scores[:R * H * T].reshape(R, H, T), ring=ring)


def judge_cross(case, route, got, failures):
    ref = DR.cross_reference(case, route, np.float64)
    f32 = DR.cross_reference(case, route, np.float32)
    rep = {}
    keys = ["out"] + (["scores"] if route != "C5" else [])
    for key in keys:
        entry, fail = DR.judge(key, got[key], ref[key], f32[key])
        rep[key] = entry
        if fail:
            failures.append(f"{route}: {fail}")
    if got["ring"] is not None:
        slots = sorted(ref["align"])
        written = np.zeros(got["ring"].shape[:3], bool)
        for s in slots:
            written[s] = True
        if not is_guard(got["ring"][~written]):
            failures.append(f"{route}: a window row outside the addressed ones lost its guard pattern")
        if slots:
            rows = np.stack([got["ring"][s] for s in slots])
            entry, fail = DR.judge("align", rows, np.stack([ref["align"][s] for s in slots]), np.stack([f32["align"][s] for s in slots]))
            rep["align"] = entry
            if fail:
                failures.append(f"{route}: {fail}")
            if np.abs(rows.astype(np.float64).sum(axis=1) - 1.0).max() > 1e-5:
                failures.append(f"{route}: an alignment row does not sum to 1")
    print(case["name"], route, json.dumps(rep))
    return rep


def same_bits(a, b, keys, what, failures):
    for key in keys:
        if a[key] is None and b[key] is None:
            continue
        if not np.array_equal(bits(a[key]), bits(b[key])):
            failures.append(f"{what}: {int((bits(a[key]) != bits(b[key])).sum())} elements of {key} differ")


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def separate_query(case):
    """q of a folded case through the separate launch the fold replaces (LayerNorm + projection GEMV, then the scale)"""
    R, d = case["R"], case["d"]
    bias = case["bq"] if case["bq"] is not None else np.zeros(d, np.float32)
    q = np.empty((R, d), np.float32)
    rc = _lib.load().wlk_diag_linear_ln(vp(case["x"]), vp(case["wq"]), vp(bias), vp(case["gamma"]), vp(case["beta"]), R, d, d, 0, vp(q))
    assert rc == 0, _lib.load().wlk_diag_last_error()
    return q * np.float32(case["scale"])


def separate_out_projection(case, att):
    d = case["d"]
    y = np.empty((1, d), np.float32)
    a = np.ascontiguousarray(att[:1])
    rc = _lib.load().wlk_diag_linear(vp(a), d, d, vp(case["wo"]), vp(case["bo"]), vp(case["resid"]), d, 1, d, d, 2, 1.0, 0, 1, vp(y))
    assert rc == 0, _lib.load().wlk_diag_last_error()
    return y


@pytest.mark.parametrize("name", DC.CROSS_NAMES)
def test_cross_attention(name):
    case = DC.build(name)
    want = DC.expected_routes(case)
    failures, rep, outs = [], {}, {}
    for route, fragment in case["refused"].items():
        rc, msg, _ = run_cross(case, route)
        if rc != WLK_ERR_ARG or fragment not in msg:
            failures.append(f"{route} must refuse with '{fragment}', answered {rc}: {msg}")
    for route in want:
        for ks in ((1, 0) if route == "C5" else (1,)):
            rc, msg, got = run_cross(case, route, k_splits=ks)
            tag = route if route != "C5" else f"C5/{'default' if ks == 0 else 'k1'}"
            if rc != 0:
                failures.append(f"{tag}: error {rc}: {msg}")
                continue
            outs[tag] = got
            rep[tag] = judge_cross(case, route, got, failures)
    # the bit-for-bit relations
    if "C1" in outs and "C4" in outs and case["n_kv"] == 1:
        same_bits(outs["C4"], outs["C1"], ("out", "scores", "ring"), "C4 against C1", failures)
    if "C2" in outs:
        rc, msg, sep = run_cross(case, "C1", q=np.ascontiguousarray(separate_query(case)))
        if rc != 0:
            failures.append(f"C1 on the separately projected query: {rc} {msg}")
        else:
            same_bits(outs["C2"], sep, ("out", "scores", "ring"), "C2 against C1 on the separately projected query", failures)
    if "C3" in outs and "C1" in outs:
        sep = dict(outs["C1"], out=separate_out_projection(case, outs["C1"]["out"]))
        same_bits(outs["C3"], sep, ("out", "scores", "ring"), "C3 against C1 + the separate out projection", failures)
    rep["routes"] = sorted(outs)
    report(name, rep)
    n_want = len(want) + (1 if "C5" in want else 0)
    assert len(outs) == n_want and not failures, "\n".join(failures)


# ----------------------------------------------------------------------------------------------------------------------
# integer and copy kernels
# ----------------------------------------------------------------------------------------------------------------------
def run_anc_updates(table, seq, n_rows):
    table = np.ascontiguousarray(table, np.uint8).copy()
    ctl = i32(np.stack([s[0] for s in seq]))
    offs = i32([s[1] for s in seq])
    rc, msg = call("A0", n_rows=n_rows, ctx_len=table.shape[1], anc=table, anc_rows=table.shape[0], n_updates=len(seq), ctl=ctl,
                   upd_offsets=offs)
    assert rc == 0, msg
    return table


@pytest.mark.parametrize("name", sorted(DC.ANC_SEQUENCES))
def test_ancestry_update_is_the_integer_model(name):
    spec = DC.ANC_SEQUENCES[name]
    seq = DC.anc_sequence(name, **spec)
    n_rows = spec["n_rows"]
    start = np.full((n_rows + 2, spec["ctx_len"]), 0xA5, np.uint8)       # stale content, two guard rows
    for n in (1, len(seq) // 2, len(seq)):
        want = start
        for ctl, off in seq[:n]:
            want = DR.anc_update(want, ctl, off, n_rows)
        got = run_anc_updates(start, seq[:n], n_rows)
        assert np.array_equal(got, want), (name, n, np.argwhere(got != want)[:8].tolist())
    # a step that is not fresh depends on the table's content: run it on a random table
    rng = np.random.default_rng(1)
    table = rng.integers(0, n_rows, start.shape).astype(np.uint8)
    assert np.array_equal(run_anc_updates(table, seq[1:2], n_rows), DR.anc_update(table, *seq[1], n_rows))
    report(name, dict(exact=True, updates=len(seq)))


def test_ancestry_update_refuses_what_it_cannot_hold():
    seq = DC.anc_sequence("x", 2, 24, 3, 1)
    for n_rows, ctx_len in ((8, 24), (2, 513)):
        table = np.zeros((8, ctx_len), np.uint8)
        rc, msg = call("A0", n_rows=n_rows, ctx_len=ctx_len, anc=table, anc_rows=8, n_updates=1, ctl=i32(seq[0][0]), upd_offsets=i32([3]))
        assert rc == WLK_ERR_ARG and "ancestry update" in msg, (rc, msg)


@pytest.mark.parametrize("d, n_tok", [(128, 1), (128, 5), (384, 3)])
def test_kv_append(d, n_tok):
    rng = np.random.default_rng(d + n_tok)
    n_rows, ctx_len, off = 3, 24, 7
    qkv = rng.standard_normal((n_rows * n_tok, 3 * d)).astype(np.float32)
    kc, vc = guard((n_rows + 1, ctx_len, d)), guard((n_rows + 1, ctx_len, d))
    want_k, want_v = DR.kv_append(kc, vc, qkv, n_tok, [off])
    rc, msg = call("K0", n_rows=n_rows, n_tok=n_tok, d=d, ctx_len=ctx_len, qkv=qkv, kcache=kc, vcache=vc, cache_floats=kc.size,
                   offsets=i32([off]))
    assert rc == 0, msg
    assert np.array_equal(bits(kc), bits(want_k)) and np.array_equal(bits(vc), bits(want_v))
    # the per-row form: its own cache row, offset and a layer offset
    rows, offs = [2, 0, 3], [23, 0, 11]
    kc, vc = guard((4, ctx_len, d)), guard((4, ctx_len, d))
    want_k, want_v = DR.kv_append(kc, vc, qkv[:3], 1, offs, rows)
    rc, msg = call("K1", n_rows=3, n_tok=1, d=d, ctx_len=ctx_len, qkv=np.ascontiguousarray(qkv[:3]), kcache=kc, vcache=vc,
                   cache_floats=kc.size, offsets=i32(offs), row_cache=i32(rows), layer_off=1028)
    assert rc == 0, msg
    assert np.array_equal(bits(kc), bits(want_k)) and np.array_equal(bits(vc), bits(want_v))


@pytest.mark.parametrize("length", [0, 1, 13, 24])
def test_kv_gather(length):
    rng = np.random.default_rng(length)
    n_layer, n_rows, ctx_len, d = 2, 5, 24, 384
    src = rng.standard_normal((n_layer, n_rows, ctx_len, d)).astype(np.float32)
    dst = guard((n_layer, n_rows, ctx_len, d))
    source = [4, 4, 0, 2, 1]
    rc, msg = call("G0", n_rows=n_rows, d=d, ctx_len=ctx_len, n_layer=n_layer, gather_len=length, kcache=src.copy(), vcache=dst,
                   cache_floats=src.size, row_cache=i32(source))
    assert rc == 0, msg
    assert np.array_equal(bits(dst[:, :, :length]), bits(DR.kv_gather(src, source, length))) and is_guard(dst[:, :, length:])


def test_ancestry_attention_equals_attention_over_the_gathered_cache():
    """a beam session both ways: every step appends position `offset` to each physical row; the gather form first moves
    every survivor's history into its row (G0 then K0), the ancestry form only updates the table (A0).  The last step's
    self-attention must give the same bits either way (S2 over the physical rows, S0 over the gathered cache)."""
    n_rows, ctx_len, d, H = 5, 160, 128, 2
    seq = DC.anc_sequence("beam_both_ways", n_rows, ctx_len, 123, 9)
    rng = np.random.default_rng(17)
    first = seq[0][1]
    phys = [np.zeros((n_rows, ctx_len, d), np.float32) for _ in range(2)]
    for c in phys:
        c[:, :first] = rng.standard_normal((n_rows, first, d)) * (DC.QK_SCALE if c is phys[0] else 1.0)
    gath = [c.copy() for c in phys]
    for ctl, off in seq:
        qkv = (rng.standard_normal((n_rows, 3 * d)) * DC.QK_SCALE).astype(np.float32)
        for i in range(2):
            dst = np.full_like(gath[i], 1e30)           # the other buffer of a session: stale behind the gathered part
            rc, msg = call("G0", n_rows=n_rows, d=d, ctx_len=ctx_len, n_layer=1, gather_len=off, kcache=gath[i], vcache=dst,
                           cache_floats=dst.size, row_cache=i32(ctl[:n_rows]))
            assert rc == 0, msg
            gath[i] = dst
        for caches in (gath, phys):
            rc, msg = call("K0", n_rows=n_rows, n_tok=1, d=d, ctx_len=ctx_len, qkv=qkv, kcache=caches[0], vcache=caches[1],
                           cache_floats=caches[0].size, offsets=i32([off]))
            assert rc == 0, msg
    table = run_anc_updates(np.full((n_rows, ctx_len), 0xA5, np.uint8), seq, n_rows)
    last = seq[-1][1]
    outs = {}
    for route, caches, extra in (("S0", gath, {}), ("S2", phys, dict(anc=table, anc_rows=n_rows))):
        out = guard((n_rows + 1, d))
        rc, msg = call(route, n_rows=n_rows, n_tok=1, d=d, n_head=H, ctx_len=ctx_len, qkv=qkv, kcache=caches[0], vcache=caches[1],
                       cache_floats=caches[0].size, offsets=i32([last]), out=out, out_floats=out.size, **extra)
        assert rc == 0 and is_guard(out[n_rows:]), (route, msg)
        outs[route] = out[:n_rows]
    assert np.array_equal(bits(outs["S0"]), bits(outs["S2"]))
    clean = [np.where(c > 1e29, 0, c).astype(np.float32) for c in gath]
    args = (qkv, clean[0], clean[1], 1, [last], H)
    entry, fail = DR.judge("out", outs["S2"], DR.self_attention(*args, np.float64), DR.self_attention(*args, np.float32))
    report("beam_both_ways", dict(S2=dict(out=entry)))
    assert fail is None, fail
    # and the table says where the gathered rows came from
    for b in range(n_rows):
        assert np.array_equal(bits(phys[0][table[b, :last + 1], np.arange(last + 1)]), bits(gath[0][b, :last + 1]))
