"""The references of tests/sf_kernel_reference.py against independent statements, on every case of
tests/sf_kernel_cases.py, without a GPU: the float64 attention against torch double with the pad-and-view rel_shift of
oracle/sortformer_oracle.py on a 2 T - 1 row table, the convolutions against torch's conv2d / conv1d / glu / batch_norm in
double; the float32 restatement against the tolerance it defines; and every deliberate mistake of the reference module
against that tolerance, on every case it applies to - a case that could not tell a mistake apart would not test it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sf_kernel_cases as SC
import sf_kernel_reference as SR
from oracle.sortformer_oracle import _rel_shift


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).double()


def refs(fn, *args, rows=None, **kw):
    """-> (float64 reference, float32 restatement, allowed error per element), of the rows `rows` selects; the restatement
    must pass its own rule"""
    ref, f32 = fn(*args, dt=np.float64, **kw), fn(*args, dt=np.float32, **kw)
    assert f32.dtype == np.float32 and ref.dtype == np.float64
    if rows is not None:
        ref, f32 = ref[rows], f32[rows]
    entry, fail = SR.judge("restatement", f32, ref, f32)
    assert fail is None and np.isfinite(entry["restatement_err"]), (entry, fail)
    return ref, f32, SR.value_tolerance(ref, f32)[0]


def caught(mutated, ref, allowed):
    """the mistake shows: somewhere it is further from the reference than a kernel may be"""
    err = SR.abs_err(mutated, ref)
    return bool((err > allowed).any()), float((err / allowed).max())


# ----------------------------------------------------------------------------------------------------------------------
def torch_attention(c):
    """NeMo's RelPositionMultiHeadAttention on every sequence of the case: matrix_bd over the 2 T - 1 rows the sequence can
    reach, shifted by pad-and-view"""
    q, k, v = t64(c["q"]), t64(c["k"]), t64(c["v"])
    out = torch.full(q.shape, float("nan"), dtype=torch.float64)
    H, dh = c["H"], c["dh"]
    zero = torch.zeros(H, dh, dtype=torch.float64)
    u = t64(c["bias_u"]) if c["bias_u"] is not None else zero
    vb = t64(c["bias_v"]) if c["bias_v"] is not None else zero
    for a, T in (c["segs"] or [(0, c["T"])]):
        qs = q[a:a + T]
        qu, qv = (qs + u).permute(1, 0, 2), (qs + vb).permute(1, 0, 2)                  # [H][T][dh]
        s = torch.matmul(qu, k[a:a + T].permute(1, 2, 0))
        if c["pos"] is not None:
            r0 = c["pos_row0"]
            pp = t64(c["pos"][r0 - (T - 1):r0 + T]).permute(1, 0, 2)                   # [H][2 T - 1][dh]
            bd = _rel_shift(torch.matmul(qv, pp.transpose(-2, -1)).unsqueeze(0))[0]
            s = s + bd[:, :, :T]
        w = torch.softmax(s * float(c["scale"]), dim=-1)
        out[a:a + T] = torch.matmul(w, v[a:a + T].permute(1, 0, 2)).permute(1, 0, 2)
    return out.numpy()


def attention_args(c):
    return (c["q"], c["k"], c["v"], c["scale"]), dict(pos=c["pos"], pos_row0=c["pos_row0"] or 0, bias_u=c["bias_u"],
                                                       bias_v=c["bias_v"], segs=c["segs"])


@pytest.mark.parametrize("name", SC.ATTENTION_NAMES)
def test_attention_reference_and_mutants(name):
    c = SC.attention_case(name)
    args, kw = attention_args(c)
    owned = SR.owned_rows(c["rows"], c["segs"])
    assert int(owned.sum()) == (sum(n for _, n in c["segs"]) if c["segs"] else c["T"])
    ref, f32, allowed = refs(SR.attention, *args, rows=owned, **kw)
    assert np.all(np.isfinite(ref))
    assert np.abs(ref - torch_attention(c)[owned]).max() <= 1e-11 * max(1.0, np.abs(ref).max())
    if c["plant"] is not None:
        assert np.abs(ref - c["v"][c["plant"]].astype(np.float64)).max() <= 1e-9
    mutants = SC.attention_mutants(c)
    assert set(mutants) <= set(SR.ATTENTION_MUTANTS)
    for m in mutants:
        hit, ratio = caught(SR.attention(*args, dt=np.float64, mutant=m, **kw)[owned], ref, allowed)
        assert hit, f"{name} cannot tell '{m}' from the reference (largest error {ratio:.3g} of the allowed)"


def test_every_attention_mutant_meets_cases():
    seen = {m: 0 for m in SR.ATTENTION_MUTANTS}
    for name in SC.ATTENTION_NAMES:
        c = SC.ATTENTION[name]
        assert c["T"] <= SC.MAX_FRAMES and c["dh"] % 4 == 0
    for name in ("t2_dh64_pos_edge", "seg3_dh64_pos_511", "t512_dh24_nopos", "t49_dh64_nopos_bias_u"):
        for m in SC.attention_mutants(SC.attention_case(name)):
            seen[m] += 1
    assert all(seen.values()), seen
    assert {f"t{T}_dh64_pos_edge" for T in SC.ATTN_T} <= set(SC.ATTENTION_NAMES)


# ----------------------------------------------------------------------------------------------------------------------
def per_session(lens):
    a = 0
    for n in lens:
        yield a, n
        a += n


@pytest.mark.parametrize("name", SC.CONV_NAMES)
def test_conv0_reference_and_mutant(name):
    c = SC.conv_case("conv0", name)
    args = (c["x"], c["w"], c["b"], c["lens"])
    ref, f32, allowed = refs(SR.conv0, *args)
    want = []
    for a, n in per_session(c["lens"]):
        y = F.relu(F.conv2d(t64(c["x"][a:a + n])[None, None], t64(c["w"]).view(c["C"], 1, 3, 3), t64(c["b"]), stride=2, padding=1))
        want.append(y[0].permute(1, 2, 0).numpy())          # [C][T1][F1] -> channels last
    want = np.concatenate(want)
    assert ref.shape == want.shape == (sum(SR.sub_len(n) for n in c["lens"]), SR.sub_len(c["F"]), c["C"])
    assert np.abs(ref - want).max() <= 1e-12
    hit, ratio = caught(SR.conv0(*args, dt=np.float64, mutant="tap_shifted"), ref, allowed)
    assert hit, f"{name} cannot tell a shifted tap from the reference ({ratio:.3g} of the allowed)"


@pytest.mark.parametrize("name", SC.CONV_NAMES)
def test_dwconv2d_reference_and_mutant(name):
    c = SC.conv_case("dwconv2d", name)
    args = (c["x"], c["w"], c["b"], c["lens"])
    ref, f32, allowed = refs(SR.dwconv2d, *args)
    C = c["C"]
    want = []
    for a, n in per_session(c["lens"]):
        x = t64(c["x"][a:a + n]).permute(2, 0, 1)[None]                                 # [1][C][T][F]
        y = F.conv2d(x, t64(c["w"]).t().reshape(C, 1, 3, 3), t64(c["b"]), stride=2, padding=1, groups=C)
        want.append(y[0].permute(1, 2, 0).numpy())
    want = np.concatenate(want)
    assert ref.shape == want.shape and np.abs(ref - want).max() <= 1e-12
    hit, ratio = caught(SR.dwconv2d(*args, dt=np.float64, mutant="tap_shifted"), ref, allowed)
    assert hit, f"{name} cannot tell a shifted tap from the reference ({ratio:.3g} of the allowed)"


@pytest.mark.parametrize("name", SC.GLU_NAMES)
def test_glu_dwconv_reference_and_mutants(name):
    c = SC.glu_case(name)
    args = (c["x"], c["w"], c["b"], c["bn_mean"], c["bn_invstd"], c["bn_w"], c["bn_b"], c["lens"])
    ref, f32, allowed = refs(SR.glu_dwconv, *args)
    d, taps = c["d"], c["taps"]
    eps = 1e-5
    var = 1.0 / t64(c["bn_invstd"]) ** 2 - eps              # the kernel is given 1 / sqrt(var + eps)
    want = []
    for a, n in per_session(c["lens"]):
        y = F.glu(t64(c["x"][a:a + n]).t()[None], dim=1)                                # [1][d][T]
        y = F.conv1d(y, t64(c["w"]).t().reshape(d, 1, taps), t64(c["b"]), padding=(taps - 1) // 2, groups=d)
        y = F.batch_norm(y, t64(c["bn_mean"]), var, t64(c["bn_w"]), t64(c["bn_b"]), training=False, eps=eps)
        want.append((y * torch.sigmoid(y))[0].t().numpy())
    want = np.concatenate(want)
    assert ref.shape == want.shape == (sum(c["lens"]), d)
    assert np.abs(ref - want).max() <= 1e-11 * max(1.0, np.abs(want).max())
    for m in ("tap_shifted", "bn_mean_sign"):
        hit, ratio = caught(SR.glu_dwconv(*args, dt=np.float64, mutant=m), ref, allowed)
        assert hit, f"{name} cannot tell '{m}' from the reference ({ratio:.3g} of the allowed)"


@pytest.mark.parametrize("name", SC.HEAD_NAMES)
def test_head_reference(name):
    c = SC.head_case(name)
    args = (c["x"], c["w1t"], c["b1"], c["w2"], c["b2"])
    ref, f32, allowed = refs(SR.head, *args)
    h = F.relu(F.linear(F.relu(t64(c["x"])), t64(c["w1t"]).t().contiguous(), t64(c["b1"])))
    want = torch.sigmoid(F.linear(h, t64(c["w2"]), t64(c["b2"]))).numpy()
    assert ref.shape == (c["T"], c["n_spk"]) and np.abs(ref - want).max() <= 1e-12
    assert 0.02 < ref.min() and ref.max() < 0.98 and ref.std() > 0.05       # not saturated: the sigmoid hides nothing
    # w1t is the transposed weight: taking it for the weight itself must show
    hit, ratio = caught(SR.head(c["x"], c["w1t"].T, c["b1"], c["w2"], c["b2"], dt=np.float64), ref, allowed)
    assert hit, ratio


@pytest.mark.parametrize("name", SC.ASSEMBLE_NAMES)
def test_assemble_reference(name):
    c = SC.assemble_case(name)
    ref = SR.assemble(c["ctx_rows"], c["chunk_rows"], c["lens"], c["chunk_lens"], c["scale"], np.float64)
    f32 = SR.assemble(c["ctx_rows"], c["chunk_rows"], c["lens"], c["chunk_lens"], c["scale"], np.float32)
    assert np.all(np.isfinite(ref)) and ref.shape == (sum(c["lens"]), c["d"])
    rows = []
    at = ck = 0
    for n, nc in zip(c["lens"], c["chunk_lens"]):
        rows += [c["ctx_rows"][at:at + n - nc], c["chunk_rows"][ck:ck + nc]]
        at, ck = at + n, ck + nc
    want = torch.cat([t64(r) for r in rows]) * float(c["scale"])
    assert np.array_equal(ref, want.numpy())
    assert np.array_equal(f32, ref.astype(np.float32))       # one rounding: the float32 product is the rounded exact one


def test_no_kind_is_left_out():
    assert len(SC.ATTENTION_NAMES) >= 80 and SC.CONV_NAMES and SC.GLU_NAMES and SC.HEAD_NAMES and SC.ASSEMBLE_NAMES
    lens = {n for name in SC.CONV_NAMES for n in SC.CONV[name][0]}
    assert {1, 2, 8, 9, 101} <= lens
    assert {SC.CONV[n][1] for n in SC.CONV_NAMES} == {128, 9, 8, 1} and {SC.CONV[n][2] for n in SC.CONV_NAMES} == {256, 96, 320}
    assert {n for name in SC.GLU_NAMES for n in SC.GLU[name][0]} == {1, 3, 37, 291}
