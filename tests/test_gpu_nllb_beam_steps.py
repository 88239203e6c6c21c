"""NLLB device beam steps on the GPU: the wide log-softmax top-k kernel through wlk_diag_topk against the float64
reference of tests/select_reference.py and, bit for bit, against the existing kernel; the ancestry step against
kv_reorder + step on a twin session; graph reuse, the state rule, argument errors; and `nllb.beam_search(device_steps=True)`
against `transformers`' sequences.

Tolerances (select_reference.value_tolerance): a log-probability may be off by 4 x the error the float32 restatement has
on the same rows, floored at 2^-22 * max(1, |reference|); for the two 256 206-wide shapes the allowance is the larger of
that and the error the EXISTING kernel (form 0, k = 8) has on the same rows.  Ids equal the reference wherever its gap to the
neighbouring ranks is an exact tie or exceeds twice the allowance; at most 2 % of the ranks of a random case may be
excluded, none of a planted one."""
import ctypes as C

import numpy as np
import pytest

import nllb_beam_standin as S
import select_reference as SR
from whisperlivekit_amd import _lib, nllb
from whisperlivekit_amd._lib import WlkError

pytestmark = pytest.mark.gpu

WLK_ERR_ARG = -1


def diag_topk(x, k, form):
    """-> (rc, log-probabilities [R, k], ids [R, k])"""
    x = np.ascontiguousarray(x, np.float32)
    R, V = x.shape
    vals = np.full((R, max(k, 1)), np.nan, np.float32)
    ids = np.full((R, max(k, 1)), -7, np.int32)
    rc = _lib.load().wlk_diag_topk(x.ctypes.data_as(C.c_void_p), R, V, k, form, vals.ctypes.data_as(C.c_void_p),
                                   ids.ctypes.data_as(C.c_void_p))
    return rc, vals, ids


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def random_rows(V, R, seed):
    return (np.random.default_rng(seed).standard_normal((R, V)) * 3).astype(np.float32)


# ---- the kernel against float64 ---------------------------------------------------------------------------------------
SHAPES = [(256206, 8, 16), (256206, 5, 10), (262144, 2, 9), (4097, 8, 16), (2003, 8, 16), (1000, 3, 16)]


@pytest.mark.parametrize("si", range(len(SHAPES)), ids=[f"v{v}_r{r}_k{k}" for v, r, k in SHAPES])
def test_wide_topk_against_float64(si):
    V, R, k = SHAPES[si]
    x = random_rows(V, R, si)
    ref_v, ref_i, gaps, _ = SR.logsoftmax_topk(x, None, k)
    f32_v, _ = SR.logsoftmax_topk_f32(x, None, k)
    allowed, e32 = SR.value_tolerance(ref_v, f32_v)
    rc, got_v, got_i = diag_topk(x, k, 1)
    assert rc == 0, _lib.load().wlk_diag_last_error()
    e_form0 = None
    if V == 256206:           # the parent's kernel on the same rows: its own error is allowed to this one too
        rc0, v0, _ = diag_topk(x, 8, 0)
        assert rc0 == 0
        e_form0 = float(SR.abs_err(v0, ref_v[:, :8]).max())
        allowed = np.maximum(allowed, e_form0)
    err = SR.abs_err(got_v, ref_v)
    print(f"wide top-k V={V} rows={R} k={k}: kernel error {err.max():.3e}, float32 restatement {e32:.3e}, "
          f"form 0 at k=8 {e_form0 if e_form0 is None else format(e_form0, '.3e')}, allowed {float(allowed.max()):.3e}, "
          f"smallest gap {gaps.min():.3e}")
    assert (err <= allowed).all(), f"value error {err.max():.3e} > allowed {float(allowed.max()):.3e}"
    decided = (gaps == 0) | (gaps > 2 * allowed)
    assert (~decided).sum() <= 0.02 * gaps.size, f"{int((~decided).sum())} of {gaps.size} ranks excluded"
    assert np.array_equal(got_i[decided], ref_i[decided]), (got_i, ref_i)


PLANTED = S.planted_rows()


@pytest.mark.parametrize("name", sorted(PLANTED))
def test_wide_topk_planted_rows(name):
    x, k, n_finite = PLANTED[name]
    ref_v, ref_i, _, _ = SR.logsoftmax_topk(x, None, k)
    f32_v, _ = SR.logsoftmax_topk_f32(x, None, k)
    rc, got_v, got_i = diag_topk(x, k, 1)
    assert rc == 0, _lib.load().wlk_diag_last_error()
    n = k if n_finite is None else n_finite
    assert np.array_equal(got_i[:, :n], ref_i[:, :n]), (got_i, ref_i)                  # exact: nothing excluded
    assert np.array_equal(got_i, S.emulate_wide_topk(x, k))
    allowed, _ = SR.value_tolerance(ref_v[:, :n], f32_v[:, :n])
    assert (SR.abs_err(got_v[:, :n], ref_v[:, :n]) <= allowed).all()
    assert (got_i[:, n:] == -1).all() and np.isneginf(got_v[:, n:]).all()              # the fill


def test_wide_topk_refusals():
    lib = _lib.load()
    rc, _, _ = diag_topk(np.zeros((1, 262145), np.float32), 4, 1)
    assert rc == WLK_ERR_ARG and b"262144" in lib.wlk_diag_last_error()
    x = random_rows(2003, 2, 0)
    assert diag_topk(x, 17, 1)[0] == WLK_ERR_ARG
    assert diag_topk(x, 9, 0)[0] == WLK_ERR_ARG                     # the existing form stops at 8 and is not rerouted
    assert diag_topk(x, 0, 1)[0] == WLK_ERR_ARG


@pytest.mark.parametrize("V", [256206, 51865, 2003])
def test_wide_topk_ranks_0_to_7_are_the_existing_kernels(V):
    x = random_rows(V, 3, 40 + V % 7)
    rc1, v1, i1 = diag_topk(x, 16, 1)
    rc0, v0, i0 = diag_topk(x, 8, 0)
    assert rc1 == 0 and rc0 == 0
    assert np.array_equal(bits(v1[:, :8]), bits(v0)) and np.array_equal(i1[:, :8], i0)


# ---- the ancestry step ------------------------------------------------------------------------------------------------
def _model(weights, max_tgt=64):
    return nllb.HipNllbModel.from_hf_state_dict(nllb.NLLB_MICRO, nllb.synth_state_dict(nllb.NLLB_MICRO, weights["seed"], weights["eos_gain"]),
                                                device=0, max_src=92, max_tgt=max_tgt)


@pytest.fixture(scope="module")
def models():
    m = {"old": _model(S.OLD_WEIGHTS), "wide": _model(S.WIDE_WEIGHTS)}
    yield m
    for v in m.values():
        v.close()


def _sources(step, rows, rng):
    if step == 0:
        return np.arange(rows)
    if step == 1:
        return np.zeros(rows, np.int64)
    if step == 2:
        return (np.arange(rows) + 1) % rows
    return rng.integers(0, rows, size=rows)           # shared and dropped ancestors


@pytest.mark.parametrize("rows,plain_first", [(2, False), (5, False), (8, False), (5, True)])
def test_ancestry_step_equals_gather_then_step(models, rows, plain_first):
    """plain_first: a `step` and a `kv_reorder` (the cache half flips) on both twins between the prompt and the first ancestry
    step, which is still `fresh` - every physical row holds its own history, whatever plain calls came between."""
    rng = np.random.default_rng(rows)
    a, b = models["old"].new_session(rows), models["old"].new_session(rows)
    try:
        src = S.KAT["beam_src1"]
        prompt = np.tile(np.asarray([[2, 1991]], np.int64), (rows, 1))
        prompt[:, 1] += np.arange(rows)                                       # every row its own history from the start
        for s in (a, b):
            s.encode(src)
            s.decode(prompt, first=True)
        if plain_first:
            tokens = rng.integers(4, 1900, size=rows)
            for s in (a, b):
                s.step(tokens, 4)
                s.kv_reorder((np.arange(rows) + 2) % rows)
        before = a.beam_stats()["ancestry_steps"]
        for step in range(24):
            k = 6 if step < 12 else 16
            sources = _sources(step, rows, rng)
            tokens = rng.integers(4, 1900, size=rows)
            lp_a, id_a = a.step_beam(tokens, sources, k)
            b.kv_reorder(sources)
            lp_b, id_b = b.step(tokens, min(k, 8))
            assert np.array_equal(bits(a.logits()), bits(b.logits())), f"step {step}: logits differ"
            n = min(k, 8)
            assert np.array_equal(bits(lp_a[:, :n]), bits(lp_b)) and np.array_equal(id_a[:, :n], id_b), f"step {step}: top-k differs"
        assert a.beam_stats()["ancestry_steps"] == before + 24
    finally:
        a.close()
        b.close()


def _case(name):
    return next(c for c in S.beam_cases() if c[0].startswith(name))


def test_graph_reuse_across_source_lengths_and_cache_halves(models):
    """One 8-row session: sentences of two source lengths (the captured step carries the source length by value), and device
    infers after host-path infers whose kv_reorder calls flipped the cache half the step graph is recorded for."""
    c3, c4 = _case("wide3"), _case("wide4")
    assert c3[4]["num_beams"] == c4[4]["num_beams"] == 8 and len(c3[2]) != len(c4[2])
    sess = models["wide"].new_session(8)
    try:
        for case, dev in ((c3, True), (c4, True), (c3, False), (c4, True), (c4, False), (c3, False), (c3, True), (c4, True)):
            _, _, src, lang, kw, want = case
            assert nllb.beam_search(sess, src, lang, device_steps=dev, **kw) == want, (case[0], dev)
        assert sess.beam_stats()["ancestry_steps"] > 0
    finally:
        sess.close()


def test_state_rule_and_arguments(models):
    m = models["old"]
    sess = m.new_session(3)
    state, arg, cap = r"error -3", r"error -1", r"error -4"
    try:
        sess.encode(S.KAT["beam_src0"])
        with pytest.raises(WlkError, match=state):
            sess.step_beam([5, 6, 7], [0, 1, 2], 4)                           # before the prompt
        start = np.full((3, 1), 2, np.int64)
        sess.decode(start, first=True)
        with pytest.raises(WlkError, match=arg):
            sess.step_beam([5, 6, 7], [0, 1, 3], 4)                           # source row out of range
        with pytest.raises(WlkError, match=arg):
            sess.step_beam([5, 6, 7], [0, -1, 2], 4)
        with pytest.raises(WlkError, match=arg):
            sess.step_beam([5, 1, 7], [0, 1, 2], 4)                           # a pad token
        with pytest.raises(WlkError, match=arg):
            sess.step_beam([5, 6, 7], [0, 1, 2], 17)
        lp = np.empty((2, 4), np.float32)
        ids = np.empty((2, 4), np.int32)
        t, s2 = np.asarray([5, 6], np.int64), np.asarray([0, 1], np.int32)
        rc = sess.lib.wlk_nllb_step_beam(sess._h, t.ctypes.data_as(C.c_void_p), s2.ctypes.data_as(C.c_void_p), 2, 4,
                                         lp.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p))
        assert rc == WLK_ERR_ARG                                              # a wrong n_rows
        assert sess.beam_stats()["ancestry_steps"] == 0
        sess.step([5, 6, 7], 2)                                               # none of the refused calls changed the state
        sess.kv_reorder([1, 1, 0])
        sess.step_beam([8, 9, 10], [2, 0, 0], 16)
        with pytest.raises(WlkError, match=state):
            sess.step([5, 6, 7], 2)
        with pytest.raises(WlkError, match=state):
            sess.decode(np.full((3, 1), 9, np.int64), first=False)
        with pytest.raises(WlkError, match=state):
            sess.kv_reorder([0, 1, 2])
        assert sess.topk(16)[1].shape == (3, 16) and sess.logits().shape == (3, nllb.NLLB_MICRO.vocab_size)
        sess.decode(start, first=True)                                        # ... and they work again
        sess.step([5, 6, 7], 2)
        sess.kv_reorder([0, 0, 1])
        sess.decode(np.full((3, 1), 9, np.int64), first=False)
        for _ in range(64 - 3):                                               # up to the end of the target context
            sess.step_beam([5, 6, 7], [0, 1, 2], 2)
        with pytest.raises(WlkError, match=cap):
            sess.step_beam([5, 6, 7], [0, 1, 2], 2)
        # THIS session - refused calls, a full context, 61 ancestry steps, a step graph recorded for k = 2 and another source
        # length - still translates correctly, through the device steps and through the host path
        _, _, src, lang, kw, want = _case("kat0")
        assert kw["num_beams"] == 3
        assert nllb.beam_search(sess, src, lang, device_steps=True, **kw) == want
        assert nllb.beam_search(sess, src, lang, device_steps=False, **kw) == want
        assert nllb.beam_search(sess, src, lang, device_steps=True, **kw) == want
    finally:
        sess.close()


def test_topk_16_of_a_session(models):
    sess = models["old"].new_session(2)
    try:
        sess.encode(S.KAT["beam_src0"])
        sess.decode(np.asarray([[2, 1990], [2, 1991]], np.int64), first=True)
        lp16, id16 = sess.topk(16)
        lp8, id8 = sess.topk(8)
        assert np.array_equal(bits(lp16[:, :8]), bits(lp8)) and np.array_equal(id16[:, :8], id8)
        assert np.array_equal(id16, S.emulate_wide_topk(sess.logits(), 16))
        with pytest.raises(WlkError, match=r"error -1"):
            sess.topk(17)
    finally:
        sess.close()


# ---- end to end -------------------------------------------------------------------------------------------------------
CASES = S.beam_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_device_steps_return_transformers_sequence(models, case):
    _, weights, src, lang, kw, want = case
    sess = models[weights].new_session(kw["num_beams"])
    try:
        assert nllb.beam_search(sess, src, lang, device_steps=True, **kw) == want
        assert sess.beam_stats()["ancestry_steps"] > 0
    finally:
        sess.close()
