"""The kernels of csrc/sortformer.hip on chosen inputs, through wlk_diag_sf_kernel (production launchers, unchanged): the
attention the Sortformer blocks and the NLLB encoder share - matrix cores (form 2) and one wave per query (form 1) - the
stem's convolutions, the Conformer convolution core, the sigmoid head and the input assembly, each against the float64
reference of tests/sf_kernel_reference.py on the cases of tests/sf_kernel_cases.py.  No model, no session.

Tolerance (tests/select_reference.py: value_tolerance): a value may be off by 4 x the error the float32 restatement has on
the same case (floor 2^-22 * max(1, |reference|)).  Every buffer is larger than what a kernel may address and arrives
filled with a NaN bit pattern: rows past the end, the pad columns of the attention output and the gap rows between
segments must still hold it, and every input must come back bit for bit.  Position rows no query of the case can reach and
the gap rows of q / k / v hold NaN: a kernel that reads one poisons its result.  Every case writes its errors to
sf_kernels_report.json in the directory WLK_REPORT_DIR names (default: test_reports/)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import sf_kernel_cases as SC
import sf_kernel_reference as SR
from whisperlivekit_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}
WLK_ERR_ARG = -1
GUARD = np.uint32(0x7FC12345)           # a NaN with a payload: reading it poisons, and it is recognisable
PAD = 4                                 # pad columns of the attention output rows


def report(key, value):
    REPORT[key] = value
    out = os.environ.get("WLK_REPORT_DIR") or os.path.join(ROOT, "test_reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "sf_kernels_report.json"), "w") as fh:
        json.dump(REPORT, fh, indent=1, sort_keys=True)


def guard(shape):
    return np.full(shape, GUARD, np.uint32).view(np.float32)


def is_guard(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint32) == GUARD))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def guarded(a, extra=3):
    """`a` flattened into a buffer with `extra` guard words behind it -> (buffer, view of the payload)"""
    a = np.ascontiguousarray(a, np.float32)
    buf = guard(a.size + extra)
    buf[:a.size] = a.reshape(-1)
    return buf, buf[:a.size].reshape(a.shape)


def call(kind, **kw):
    """-> (rc, message).  Arrays are passed by pointer (in / out buffers are changed in place), (array, float offset) pairs
    as a pointer into the array, lists as the struct's integer tables, numbers by value."""
    a = _lib.DiagSfKernelArgs()
    a.kind = kind
    keep = []
    for key, val in kw.items():
        if val is None:
            continue
        if isinstance(val, tuple):
            arr, off = val
            keep.append(arr)
            setattr(a, key, arr.ctypes.data + 4 * off)
        elif isinstance(val, np.ndarray):
            assert val.flags["C_CONTIGUOUS"] and val.dtype == np.float32, key
            keep.append(val)
            setattr(a, key, val.ctypes.data)
        elif isinstance(val, list):
            for i, x in enumerate(val):
                getattr(a, key)[i] = int(x)
        else:
            setattr(a, key, val)
    lib = _lib.load()
    rc = lib.wlk_diag_sf_kernel(C.byref(a))
    msg = "" if rc == 0 else lib.wlk_diag_last_error().decode()
    if rc not in (0, WLK_ERR_ARG):      # a HIP error: the device's state is unknown, nothing more is launched on it
        pytest.exit(f"wlk_diag_sf_kernel: error {rc}: {msg}", returncode=3)
    return rc, msg


def judge(name, tag, got, ref, f32, rep, failures):
    entry, fail = SR.judge(tag, got, ref, f32)
    rep[tag] = entry
    print(name, tag, json.dumps(entry))
    if fail:
        failures.append(f"{name}: {fail}")


# ----------------------------------------------------------------------------------------------------------------------
# attention
# ----------------------------------------------------------------------------------------------------------------------
def run_attention(case, form, **override):
    """q | k | v interleaved in one buffer of row stride 3 H dh, as the projection GEMM leaves them; out rows H dh + 4 apart.
    -> (rc, message, out [rows][H][dh])"""
    c = case
    H, dh, rows = c["H"], c["dh"], c["rows"]
    W = H * dh
    qkv = guard((rows + 2, 3 * W))
    for i, key in enumerate("qkv"):
        qkv[:rows, i * W:(i + 1) * W] = c[key].reshape(rows, W)
    sent = qkv.copy()
    out = guard((rows + 2, W + PAD))
    kw = dict(T=c["T"], n_head=H, dh=dh, scale=float(c["scale"]), form=form, ldq=3 * W, ldk=3 * W, ldv=3 * W, ldo=W + PAD,
              q=(qkv, 0), k=(qkv, W), v=(qkv, 2 * W), q_floats=qkv.size, k_floats=qkv.size - W, v_floats=qkv.size - 2 * W,
              out=out, out_floats=out.size, bias_u=c["bias_u"], bias_v=c["bias_v"])
    pos = pos_sent = None
    if c["pos"] is not None:
        n = c["pos"].shape[0]
        pos = guard((n + 1, W + PAD))
        pos[:n, :W] = c["pos"].reshape(n, W)
        pos_sent = pos.copy()
        kw.update(pos=pos, pos_floats=pos.size, ldp=W + PAD, pos_row0=c["pos_row0"], pos_rows=n)
    if c["segs"] is not None:
        kw.update(n_seg=len(c["segs"]), seg_start=[a for a, _ in c["segs"]], seg_T=[n for _, n in c["segs"]])
    kw.update(override)
    rc, msg = call(_lib.SFK_ATTENTION, **kw)
    if rc == 0:
        owned = SR.owned_rows(rows, c["segs"])
        assert is_guard(out[rows:]), f"form {form} wrote behind its {rows} output rows"
        assert is_guard(out[:, W:]), f"form {form} wrote into the pad columns of out"
        assert is_guard(out[:rows][~owned]), f"form {form} wrote into a gap row between segments"
        assert np.array_equal(bits(qkv), bits(sent)), f"form {form} changed q / k / v"
        assert pos is None or np.array_equal(bits(pos), bits(pos_sent)), f"form {form} changed the pos table"
    else:
        assert is_guard(out), f"a refused call (form {form}) touched out"
    return rc, msg, out[:rows, :W].reshape(rows, H, dh)


def attention_refs(c):
    args = (c["q"], c["k"], c["v"], c["scale"])
    kw = dict(pos=c["pos"], pos_row0=c["pos_row0"] or 0, bias_u=c["bias_u"], bias_v=c["bias_v"], segs=c["segs"])
    own = SR.owned_rows(c["rows"], c["segs"])
    return SR.attention(*args, dt=np.float64, **kw)[own], SR.attention(*args, dt=np.float32, **kw)[own], own


@pytest.mark.parametrize("name", SC.ATTENTION_NAMES)
def test_attention(name):
    c = SC.attention_case(name)
    ref, f32, own = attention_refs(c)
    failures, rep, outs = [], {}, {}
    for form in ((2,) if c["segs"] is not None else (1, 2)):
        rc, msg, out = run_attention(c, form)
        if rc != 0:
            failures.append(f"form {form}: error {rc}: {msg}")
            continue
        outs[form] = out
        judge(name, f"form{form}", out[own], ref, f32, rep, failures)
        if c["plant"] is not None and np.abs(out.astype(np.float64) - c["v"][c["plant"]]).max() > 1e-6 * np.abs(c["v"]).max():
            failures.append(f"form {form}: row i is not the value row min(i + {SC.PLANT_OFFSET}, T - 1)")
    if c["segs"] is None:
        rc, msg, _ = run_attention(c, 1, n_seg=1, seg_start=[0], seg_T=[c["T"]])
        if rc != WLK_ERR_ARG or "segments" not in msg:
            failures.append(f"form 1 must refuse segments, answered {rc}: {msg}")
    elif 2 in outs:
        # the arithmetic of a segment is that of the same sequence alone
        for s, (a, n) in enumerate(c["segs"]):
            rc, msg, alone = run_attention(SC.attention_alone(c, s), 2)
            if rc != 0:
                failures.append(f"segment {s} alone: error {rc}: {msg}")
            elif not np.array_equal(bits(alone), bits(outs[2][a:a + n])):
                failures.append(f"segment {s} (T = {n}) differs from the same sequence alone in "
                                f"{int((bits(alone) != bits(outs[2][a:a + n])).sum())} elements")
    report("attention/" + name, rep)
    assert len(outs) == (1 if c["segs"] is not None else 2) and not failures, "\n".join(failures)


def test_attention_default_form_is_one_of_the_two():
    c = SC.attention_case("t65_dh64_pos_edge")
    outs = [run_attention(c, form) for form in (0, 1, 2)]
    assert all(rc == 0 for rc, _, _ in outs), [m for _, m, _ in outs]
    assert any(np.array_equal(bits(outs[0][2]), bits(o)) for _, _, o in outs[1:])


ATTENTION_REFUSALS = [
    ("T = 513", dict(T=513), "T in [1, 512]"),
    ("dh = 6", dict(dh=6), "dh a multiple of 4"),
    ("dh = 68", dict(dh=68), "dh a multiple of 4"),
    ("dh = 0", dict(dh=0), "dh a multiple of 4"),
    ("n_seg = 9", dict(n_seg=9), "n_seg in [0, 8]"),
    ("seg_T = 0", dict(n_seg=2, seg_start=[0, 20], seg_T=[20, 0]), "seg_T in [1, T]"),
    ("seg_T > T", dict(n_seg=2, seg_start=[0, 20], seg_T=[20, 50]), "seg_T in [1, T]"),
    ("a segment past its buffer", dict(n_seg=2, seg_start=[0, 40], seg_T=[20, 20]), "a segment lies past"),
    ("pos_row0 < T - 1", dict(pos_row0=47), "pos_row0 below T - 1"),
    ("a pos table with too few rows", dict(pos_rows=96), "at least 2 pos_row0 + 1 rows"),
    ("form 1 with segments", dict(form=1, n_seg=1, seg_start=[0], seg_T=[49]), "does not take segments"),
    ("an unknown form", dict(form=3), "form is 0"),
]


@pytest.mark.parametrize("what, override, fragment", ATTENTION_REFUSALS, ids=[r[0] for r in ATTENTION_REFUSALS])
def test_attention_refusals(what, override, fragment):
    c = SC.attention_case("t49_dh64_pos_edge")
    override = dict(override)
    rc, msg, _ = run_attention(c, override.pop("form", 2), **override)        # (run_attention checks that out is untouched)
    assert rc == WLK_ERR_ARG and fragment in msg, (what, rc, msg)


# ----------------------------------------------------------------------------------------------------------------------
# the other kernels
# ----------------------------------------------------------------------------------------------------------------------
def run_rows(kind, name, x, out_shape, ref, f32, exact=False, **kw):
    """one call of a kind whose input is `x` and whose output has `out_shape`; both behind guard words"""
    xin, _ = guarded(x)
    sent = xin.copy()
    n_out = int(np.prod(out_shape))
    out = guard(n_out + 5)
    rc, msg = call(kind, out=out, out_floats=out.size, **{"in": xin}, in_floats=xin.size, **kw)
    assert rc == 0, msg
    assert is_guard(out[n_out:]), "wrote behind its output"
    assert np.array_equal(bits(xin), bits(sent)), "changed its input"
    got = out[:n_out].reshape(out_shape)
    failures, rep = [], {}
    judge(name, "out", got, ref, f32, rep, failures)
    if exact and not np.array_equal(bits(got), bits(f32)):
        failures.append(f"{name}: {int((bits(got) != bits(f32)).sum())} elements are not the float32 product")
    report(name, rep)
    assert not failures, "\n".join(failures)
    return got


@pytest.mark.parametrize("kind", ["conv0", "dwconv2d"])
@pytest.mark.parametrize("name", SC.CONV_NAMES)
def test_stem_convolutions(name, kind):
    c = SC.conv_case(kind, name)
    fn = SR.conv0 if kind == "conv0" else SR.dwconv2d
    args = (c["x"], c["w"], c["b"], c["lens"])
    ref, f32 = fn(*args, dt=np.float64), fn(*args, dt=np.float32)
    run_rows(_lib.SFK_CONV0 if kind == "conv0" else _lib.SFK_DWCONV2D, f"{kind}/{name}", c["x"], ref.shape, ref, f32,
             n_sess=len(c["lens"]), len=list(c["lens"]), F=c["F"], C=c["C"], w=c["w"], b=c["b"])


@pytest.mark.parametrize("name", SC.GLU_NAMES)
def test_glu_dwconv(name):
    c = SC.glu_case(name)
    args = (c["x"], c["w"], c["b"], c["bn_mean"], c["bn_invstd"], c["bn_w"], c["bn_b"], c["lens"])
    ref, f32 = SR.glu_dwconv(*args, dt=np.float64), SR.glu_dwconv(*args, dt=np.float32)
    run_rows(_lib.SFK_GLU_DWCONV, f"glu_dwconv/{name}", c["x"], ref.shape, ref, f32, n_sess=len(c["lens"]), len=list(c["lens"]),
             d=c["d"], taps=c["taps"], w=c["w"], b=c["b"], bn_mean=c["bn_mean"], bn_invstd=c["bn_invstd"], bn_w=c["bn_w"],
             bn_b=c["bn_b"])


@pytest.mark.parametrize("name", SC.HEAD_NAMES)
def test_head(name):
    c = SC.head_case(name)
    args = (c["x"], c["w1t"], c["b1"], c["w2"], c["b2"])
    ref, f32 = SR.head(*args, dt=np.float64), SR.head(*args, dt=np.float32)
    run_rows(_lib.SFK_HEAD, f"head/{name}", c["x"], ref.shape, ref, f32, T=c["T"], d=c["d"], n_spk=c["n_spk"], w=c["w1t"],
             b=c["b1"], w2=c["w2"], b2=c["b2"])


@pytest.mark.parametrize("name", SC.ASSEMBLE_NAMES)
def test_assemble(name):
    c = SC.assemble_case(name)
    args = (c["ctx_rows"], c["chunk_rows"], c["lens"], c["chunk_lens"], c["scale"])
    ref, f32 = SR.assemble(*args, dt=np.float64), SR.assemble(*args, dt=np.float32)
    chunk, _ = guarded(c["chunk_rows"])
    sent = chunk.copy()
    run_rows(_lib.SFK_ASSEMBLE, f"assemble/{name}", c["ctx_rows"], ref.shape, ref, f32, exact=True, n_sess=len(c["lens"]),
             len=list(c["lens"]), len2=list(c["chunk_lens"]), d=c["d"], scale=float(c["scale"]), in2=chunk, in2_floats=chunk.size)
    assert np.array_equal(bits(chunk), bits(sent))


def test_other_kinds_refuse_what_their_buffers_cannot_hold():
    c = SC.conv_case("conv0", "three_f1_c320")
    x, out = np.ascontiguousarray(c["x"]), guard(64)
    for kind, kw, fragment in (
            (_lib.SFK_CONV0, dict(n_sess=3, len=[8, 1, 3], F=1, C=320, w=c["w"], b=c["b"]), "lie past in / out"),
            (_lib.SFK_CONV0, dict(n_sess=9, len=[1] * 8, F=1, C=320, w=c["w"], b=c["b"]), "n_sess in [1, 8]"),
            (_lib.SFK_DWCONV2D, dict(n_sess=1, len=[0], F=1, C=320, w=c["w"], b=c["b"]), "a session length"),
            (_lib.SFK_GLU_DWCONV, dict(n_sess=1, len=[2], d=4, taps=8, w=c["w"], b=c["b"]), "taps odd"),
            (_lib.SFK_HEAD, dict(T=100, d=4, n_spk=4, w=c["w"], b=c["b"], w2=c["w"], b2=c["b"]), "lie past in / out"),
            (_lib.SFK_ASSEMBLE, dict(n_sess=1, len=[2], len2=[3], d=4, scale=1.0), "chunk rows in [0, len]"),
            (17, dict(), "unknown kind")):
        rc, msg = call(kind, out=out, out_floats=out.size, **{"in": x}, in_floats=x.size, **kw)
        assert rc == WLK_ERR_ARG and fragment in msg and is_guard(out), (kind, rc, msg)
