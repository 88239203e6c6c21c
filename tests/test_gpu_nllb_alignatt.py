"""AlignAtt streaming translation on the GPU.

1. the read-out kernel alone (wlk_diag_nllb_align) against numpy float64 - cases, tolerance and exemption rule in
   tests/nllb_align_cases.py (select_reference.value_tolerance: 4 x the float32 restatement's error, floored at 2^-22;
   positions exact wherever the float64 margin is 0 or exceeds twice that; no planted row and at most 2 % of a shape's random
   rows exempt);
2. step_align on the gain-8 micro weights against `transformers` (tests/golden/nllb_align_kat.npz): p within 2e-4 absolute
   (ENC_ATOL of tests/test_nllb.py, the project's bound for this network's O(1) outputs at this shape), positions identical on
   every step (the generator proved every gap > 4e-4); the 600M shape within 1e-3 (that shape's existing bound), positions
   where the stored gap exceeds 2e-3;
3. nothing else moves: step_align's top-k is bit for bit step's, generate is unchanged, no graph without heads;
4. the library loop == the Python loop == the stored outcomes; graph reuse; state and argument errors;
5. HipAlignAttTranslation on the device against HipOnlineTranslation over the same words."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import nllb_align_cases as AC
import nllb_align_standin as A
from whisperlivekit_amd import _lib, nllb
from whisperlivekit_amd._lib import WlkError

pytestmark = pytest.mark.gpu

KAT = H.golden_npz("nllb_align_kat.npz")
N_CASES = int(KAT["n_cases"])
CFG = nllb.NLLB_MICRO
HEADS = [tuple(h) for h in KAT["heads"].tolist()]
WLK_ERR_ARG, WLK_ERR_STATE = -1, -3
P_ATOL, P_ATOL_600M, GAP_600M = 2e-4, 1e-3, 2e-3
GUARD = 8


def err_code(excinfo):
    return int(str(excinfo.value).split("wlk_hip error ")[1].split(":")[0])


@pytest.fixture(scope="module")
def micro_hip():
    m = nllb.HipNllbModel.from_hf_state_dict(CFG, A.align_gain_state_dict(CFG, 0), device=0, max_src=92, max_tgt=64)
    yield m
    m.close()


# ---- 1. the kernel alone ----------------------------------------------------------------------------------------------
def diag_align(probs, lo, hi, limit):
    """-> (rc, p, pos, prob, mass); every output sits between NaN (int: -7) guard cells that must come back untouched"""
    probs = np.ascontiguousarray(probs, np.float32)
    n, rows, S = probs.shape
    p = np.full(rows * S + 2 * GUARD, np.nan, np.float32)
    pos = np.full(rows + 2 * GUARD, -7, np.int32)
    prob = np.full(rows + 2 * GUARD, np.nan, np.float32)
    mass = np.full(rows + 2 * GUARD, np.nan, np.float32)
    at = lambda a: C.c_void_p(a.ctypes.data + GUARD * a.itemsize)      # noqa: E731
    rc = _lib.load().wlk_diag_nllb_align(probs.ctypes.data_as(C.c_void_p), n, rows, S, lo, hi, limit, at(p), at(pos), at(prob),
                                         at(mass))
    for a, fill in ((p, None), (pos, -7), (prob, None), (mass, None)):
        edge = np.concatenate([a[:GUARD], a[-GUARD:]])
        assert np.isnan(edge).all() if fill is None else (edge == fill).all(), "a guard cell was written"
    return rc, p[GUARD:-GUARD].reshape(rows, S), pos[GUARD:-GUARD], prob[GUARD:-GUARD], mass[GUARD:-GUARD]


@pytest.mark.parametrize("si", range(len(AC.SHAPES)), ids=["a%d_r%d_s%d" % s for s in AC.SHAPES])
def test_readout_kernel_against_float64(si):
    exempt = random_rows = 0
    for name, kind, probs, lo, hi, limit in AC.cases_of(si):
        rc, p, pos, prob, mass = diag_align(probs, lo, hi, limit)
        assert rc == 0, (name, _lib.load().wlk_diag_last_error())
        report, failures, n_exempt, rows = AC.compare(kind, probs, lo, hi, limit, (p, pos, prob, mass))
        print(f"{AC.SHAPES[si]} {name}: window [{lo}, {hi}) limit {limit}: p error {report['p']['kernel_err']:.3e} (float32 "
              f"restatement {report['p']['restatement_err']:.3e}, allowed {report['p']['allowed']:.3e}), mass error "
              f"{report['mass']['kernel_err']:.3e} (allowed {report['mass']['allowed']:.3e}), smallest margin "
              f"{report['margin_min']:.3e}, exempt rows {n_exempt}")
        assert not failures, (name, failures)
        if lo >= hi:
            assert (pos == -1).all() and (prob == 0).all(), name
        if kind == "random":
            exempt, random_rows = exempt + n_exempt, random_rows + rows
    assert exempt <= 0.02 * random_rows, f"{exempt} of {random_rows} random rows exempt"


def test_readout_kernel_refuses_bad_arguments():
    good = AC.random_probs(2, 2, 9, 0)
    big = np.zeros(65 * 9 * 513, np.float32)               # large enough for every refused shape, were one to be read
    lib = _lib.load()
    for n, rows, S, lo, hi, limit in [(0, 2, 9, 1, 8, 0), (65, 2, 9, 1, 8, 0), (2, 0, 9, 1, 8, 0), (2, 9, 9, 1, 8, 0), (2, 2, 0, 0, 0, 0),
                                      (2, 2, 513, 1, 8, 0), (2, 2, 9, -1, 8, 0), (2, 2, 9, 1, 10, 0), (2, 2, 9, 1, 8, -1), (2, 2, 9, 1, 8, 10)]:
        buf = np.full(8 * 600, np.nan, np.float32)
        ib = np.full(16, -7, np.int32)
        rc = lib.wlk_diag_nllb_align(big.ctypes.data_as(C.c_void_p), n, rows, S, lo, hi, limit,
                                     buf.ctypes.data_as(C.c_void_p), ib.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p),
                                     buf.ctypes.data_as(C.c_void_p))
        assert rc == WLK_ERR_ARG, (n, rows, S, lo, hi, limit)
        assert np.isnan(buf).all() and (ib == -7).all()
    rc, *_ = diag_align(good, 1, 8, 9)
    assert rc == 0


# ---- 2. step_align against transformers ---------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(N_CASES))
def test_step_align_matches_transformers(micro_hip, ci):
    sess = micro_hip.new_session(1)
    try:
        sess.set_alignment_heads(HEADS)
        worst = A.follow_greedy(sess, KAT, f"c{ci}_", P_ATOL)
        print(f"case {ci} (S = {len(KAT[f'c{ci}_src'])}): largest |p - p64| {worst:.3e} (bound {P_ATOL:.0e}), smallest stored gap "
              f"{float(KAT[f'c{ci}_gap'].min()):.3e}")
    finally:
        sess.close()


def test_step_align_matches_transformers_at_the_600m_shape():
    cfg = nllb.NLLB_200_DISTILLED_600M
    model = nllb.HipNllbModel.from_hf_state_dict(cfg, A.align_gain_state_dict(cfg, int(KAT["big_seed"])), device=0, max_src=64,
                                                 max_tgt=32)
    sess = model.new_session(1)
    try:
        sess.set_alignment_heads([tuple(h) for h in KAT["big_heads"].tolist()])
        worst = A.follow_greedy(sess, KAT, "big_", P_ATOL_600M, min_gap=GAP_600M)
        print(f"600M shape: largest |p - p64| {worst:.3e} (bound {P_ATOL_600M:.0e}), smallest stored gap {float(KAT['big_gap'].min()):.3e}")
    finally:
        sess.close()
        model.close()


# ---- 3. nothing else moves ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 3])
def test_step_align_leaves_the_step_results_bit_for_bit(micro_hip, rows):
    src = KAT["c3_src"]
    S = len(src)
    a, b = micro_hip.new_session(rows), micro_hip.new_session(rows)
    try:
        a.set_alignment_heads(HEADS)
        prompt = np.asarray([[2, 1991 + r] for r in range(rows)], np.int64)
        for s in (a, b):
            s.encode(src)
            s.decode(prompt, first=True)
        toks = [40 + r for r in range(rows)]
        for step in range(4):
            lp_a, id_a, pos, prob, mass = a.step_align(toks, 4, 1, S - 1, S // 2)
            lp_b, id_b = b.step(toks, 4)
            assert np.array_equal(lp_a.view(np.uint32), lp_b.view(np.uint32)) and np.array_equal(id_a, id_b), f"step {step}"
            p = a.alignment()
            assert p.shape == (rows, S) and ((pos >= 1) & (pos < S - 1)).all()
            for r in range(rows):       # the results travel in the host-coherent block: they are the exported p's
                assert pos[r] == 1 + int(np.argmax(p[r, 1:S - 1])) and prob[r] == p[r, pos[r]]
                assert abs(mass[r] - p[r, S // 2:].sum(dtype=np.float64)) < 1e-6
            if rows > 1:
                assert not np.array_equal(p[0], p[1])
            toks = id_a[:, 0].tolist()
        # the two step kinds share the cache: a plain step after align steps continues the same hypotheses
        lp_a, id_a = a.step(toks, 4)
        lp_b, id_b = b.step(toks, 4)
        assert np.array_equal(lp_a.view(np.uint32), lp_b.view(np.uint32)) and np.array_equal(id_a, id_b)
        assert a.align_stats() == {"align_steps": 4, "graph_captures": 1}
    finally:
        a.close(); b.close()


def test_generate_is_unchanged_and_records_no_align_graph(micro_hip):
    kat = H.golden_npz("nllb_kat.npz")
    with_heads, without = micro_hip.new_session(1), micro_hip.new_session(1)
    try:
        with_heads.set_alignment_heads(HEADS)
        for ci in (1, 2, 3):
            lang, max_new = (int(v) for v in kat["cases"][ci])
            want = nllb.generate(without, kat[f"src{ci}"], lang, max_new_tokens=max_new)
            assert nllb.generate(with_heads, kat[f"src{ci}"], lang, max_new_tokens=max_new) == want
        assert without.align_stats() == {"align_steps": 0, "graph_captures": 0}
        assert with_heads.align_stats() == {"align_steps": 0, "graph_captures": 0}
    finally:
        with_heads.close(); without.close()


# ---- 4. the loops -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(N_CASES))
def test_device_loop_equals_python_loop_equals_the_stored_outcomes(micro_hip, ci):
    prefix = f"c{ci}_"
    src, lang = KAT[prefix + "src"], int(KAT[prefix + "lang"])
    dev, py = micro_hip.new_session(1), micro_hip.new_session(1)
    try:
        for s in (dev, py):
            s.set_alignment_heads(HEADS)
        for k, n_acc, thr, final, committed, max_new, want_ids, want_align, want_why in A.settings_of(KAT, prefix):
            kw = dict(committed=committed, n_accessible=n_acc, threshold=thr, final=final, max_new_tokens=max_new)
            got_dev = nllb.generate_alignatt(dev, src, lang, device_loop=True, **kw)
            got_py = nllb.generate_alignatt(py, src, lang, device_loop=False, **kw)
            assert got_dev == got_py, f"setting {k}"
            assert got_dev == (want_ids, want_align, want_why), f"setting {k}"
        # updates that differ only in n_accessible / threshold / the committed prefix replay ONE recording
        assert dev.align_stats()["graph_captures"] == 1 and py.align_stats()["graph_captures"] == 1
        assert dev.align_stats()["align_steps"] == py.align_stats()["align_steps"] > 0
    finally:
        dev.close(); py.close()


def test_eos_and_context_stops_agree_between_the_loops(micro_hip):
    """</s> never wins on these weights, so the loops are handed a token of the greedy run as the end marker; the context
    stop comes from max_tgt = 64."""
    prefix = "c3_"
    src, lang, greedy = KAT[prefix + "src"], int(KAT[prefix + "lang"]), KAT[prefix + "greedy"].tolist()
    marker = greedy[3]
    assert marker != greedy[0] and greedy.index(marker) == 3
    dev, py = micro_hip.new_session(1), micro_hip.new_session(1)
    try:
        for s in (dev, py):
            s.set_alignment_heads(HEADS)
            s.encode(src)
        S = len(src)
        for final, n_acc, committed in [(True, S, 0), (False, S, 0), (True, 2, 2), (False, 3, 0)]:
            prompt = [2, lang] + greedy[:committed]
            got_dev = dev.generate_alignatt_loop(prompt, n_acc, 0, final, marker, 12)
            got_py = nllb.alignatt_loop(py, prompt, S, n_acc, 0, final, marker, 12)
            assert got_dev == got_py, (final, n_acc, committed)
            if n_acc == S or final:
                assert got_dev == (greedy[committed:3], KAT[prefix + "pos"][committed:3].tolist(), "eos")
            else:
                assert got_dev[2] == "attention"
        got_dev = dev.generate_alignatt_loop([2, lang], S, 0, True, CFG.eos_token_id, 199)
        got_py = nllb.alignatt_loop(py, [2, lang], S, S, 0, True, CFG.eos_token_id, 199)
        assert got_dev == got_py and got_dev[2] == "context" and len(got_dev[0]) == 63
    finally:
        dev.close(); py.close()


def test_graph_reuse_across_updates_and_source_lengths(micro_hip):
    sess = micro_hip.new_session(1)
    try:
        sess.set_alignment_heads(HEADS)
        src, lang = KAT["c4_src"], int(KAT["c4_lang"])
        for n_acc, thr in [(64, 0), (40, 2), (20, 1), (64, 5)]:
            nllb.generate_alignatt(sess, src, lang, n_accessible=n_acc, threshold=thr, final=False, max_new_tokens=6)
            assert sess.align_stats()["graph_captures"] == 1
        nllb.generate_alignatt(sess, KAT["c2_src"], int(KAT["c2_lang"]), n_accessible=17, threshold=0, final=False, max_new_tokens=6)
        assert sess.align_stats()["graph_captures"] == 2             # another source length: one more recording
        nllb.generate_alignatt(sess, KAT["c2_src"], int(KAT["c2_lang"]), n_accessible=9, threshold=0, final=True, max_new_tokens=6)
        assert sess.align_stats()["graph_captures"] == 2
        sess.set_alignment_heads(HEADS[:1])                          # the head count travels by value: a new recording
        nllb.generate_alignatt(sess, KAT["c2_src"], int(KAT["c2_lang"]), n_accessible=9, threshold=0, final=True, max_new_tokens=2)
        assert sess.align_stats()["graph_captures"] == 3
    finally:
        sess.close()


def test_state_and_argument_errors(micro_hip):
    sess, beams = micro_hip.new_session(1), micro_hip.new_session(2)
    try:
        for bad in ([(2, 0)], [(0, 2)], [(-1, 0)], [(0, 0), (0, 0)], [(0, 0)] * 65):
            with pytest.raises(WlkError) as e:
                sess.set_alignment_heads(bad)
            assert err_code(e) == WLK_ERR_ARG, bad
        src = KAT["c2_src"]
        S = len(src)
        sess.encode(src)
        sess.decode(np.asarray([[2]], np.int64), first=True)
        with pytest.raises(WlkError) as e:                            # before heads are set
            sess.step_align([1992], 1, 1, S - 1, 0)
        assert err_code(e) == WLK_ERR_STATE
        with pytest.raises(WlkError) as e:
            sess.generate_alignatt_loop([2, 1992], S, 0, False, 2, 4)
        assert err_code(e) == WLK_ERR_STATE
        with pytest.raises(WlkError) as e:
            sess.alignment()
        assert err_code(e) == WLK_ERR_STATE
        sess.set_alignment_heads(HEADS)
        for lo, hi, limit in [(-1, S - 1, 0), (1, S + 1, 0), (1, S - 1, -1), (1, S - 1, S + 1)]:
            with pytest.raises(WlkError) as e:
                sess.step_align([1992], 1, lo, hi, limit)
            assert err_code(e) == WLK_ERR_ARG, (lo, hi, limit)
        for k in (0, 9):
            with pytest.raises(WlkError) as e:
                sess.step_align([1992], k, 1, S - 1, 0)
            assert err_code(e) == WLK_ERR_ARG
        with pytest.raises(WlkError) as e:                            # a one-token prompt
            sess.generate_alignatt_loop([2], S, 0, False, 2, 4)
        assert err_code(e) == WLK_ERR_ARG
        with pytest.raises(WlkError) as e:
            sess.generate_alignatt_loop([2, 1992], S + 1, 0, False, 2, 4)
        assert err_code(e) == WLK_ERR_ARG
        sess.step_align([1992], 1, 1, S - 1, S)                       # the refused calls left the session usable
        assert sess.alignment().shape == (1, S)
        sess.set_alignment_heads([])                                  # switched off again
        with pytest.raises(WlkError) as e:
            sess.step_align([5], 1, 1, S - 1, 0)
        assert err_code(e) == WLK_ERR_STATE
        fresh = micro_hip.new_session(1)
        try:
            fresh.set_alignment_heads(HEADS)
            fresh.encode(src)
            with pytest.raises(WlkError) as e:                        # before the decoder prompt
                fresh.step_align([1992], 1, 1, S - 1, 0)
            assert err_code(e) == WLK_ERR_STATE
        finally:
            fresh.close()
        # after an ancestry step the cache rows are no longer the hypotheses
        beams.set_alignment_heads(HEADS)
        beams.encode(src)
        beams.decode(np.asarray([[2, 1992], [2, 1992]], np.int64), first=True)
        beams.step_align([7, 8], 2, 1, S - 1, 0)
        beams.step_beam([9, 10], [1, 0], 4)
        with pytest.raises(WlkError) as e:
            beams.step_align([11, 12], 2, 1, S - 1, 0)
        assert err_code(e) == WLK_ERR_STATE
        with pytest.raises(WlkError) as e:                            # the loop is for 1-row sessions
            beams.generate_alignatt_loop([2, 1992], S, 0, False, 2, 4)
        assert err_code(e) == WLK_ERR_ARG
    finally:
        sess.close(); beams.close()


# ---- 5. the session object on the device ----------------------------------------------------------------------------------
def test_translation_session_on_the_device(micro_hip):
    """A 12-word sentence word by word plus a tail: append-only text, the final = generate_alignatt(final=True) from the same
    prefix, and fewer decoder steps than HipOnlineTranslation over the same words (counters, not time)."""
    from test_translation import WordTokenizer, words
    align_steps, local_steps, report = A.stream_twelve_words(micro_hip, WordTokenizer(), words)
    print(report)
    assert 0 < align_steps < local_steps
