"""AlignAtt through the stacked batch on the GPU.

1. the ragged read-out kernel alone (wlk_diag_nllb_align_rows) against numpy float64, row by row through
   tests/nllb_align_cases.py `compare` (select_reference.value_tolerance; positions exact where decided), NO exempt row: on
   these inputs the float32 restatement passes with 0 failures and 0 exempt rows out of 63, and the kernel is held to that;
   planted rows; NaN behind every row's length;
2. step_align on the gain-8 micro weights against `transformers` (tests/golden/nllb_align_kat.npz), six cases in six slots,
   row counts 6 .. 1, two slot orders: p within 2e-4 of p64; the 600M shape in slot 5 within 1e-3;
3. nothing else moves: step_align's top-k is bit for bit step's on a twin batch; generate_batch with heads set;
4. rows are independent: a slot's bits alone and among seven neighbours;
5. prefill against token-by-token steps and against a 1-row session; four prompts in one call against four calls;
6. generate_alignatt_batch over the library == the 78 stored outcomes == generate_alignatt on a session; graph captures;
7. errors; 8. eight stacked HipAlignAttTranslation sessions on eight threads."""
import ctypes as C
import threading

import numpy as np
import pytest

import helpers as H
import nllb_align_cases as AC
import nllb_align_standin as A
import nllb_alignatt_batch_standin as B
from whisperlivekit_amd import _lib, nllb
from whisperlivekit_amd import translation as T
from whisperlivekit_amd._lib import WlkError
from whisperlivekit_amd.policy import ASRToken

pytestmark = pytest.mark.gpu

KAT = H.golden_npz("nllb_align_kat.npz")
N_CASES = int(KAT["n_cases"])
CFG = nllb.NLLB_MICRO
HEADS = [tuple(h) for h in KAT["heads"].tolist()]
WLK_ERR_ARG, WLK_ERR_STATE, WLK_ERR_CAPACITY = -1, -3, -4
P_ATOL, P_ATOL_600M, GAP_600M = 2e-4, 1e-3, 2e-3      # tests/test_gpu_nllb_alignatt.py's bounds for the session
STRIDE = 512
SENTINEL = np.float32(-5.0)
START = CFG.decoder_start_token_id


def err_code(excinfo):
    return int(str(excinfo.value).split("wlk_hip error ")[1].split(":")[0])


@pytest.fixture(scope="module")
def micro_hip():
    m = nllb.HipNllbModel.from_hf_state_dict(CFG, A.align_gain_state_dict(CFG, 0), device=0, max_src=92, max_tgt=64)
    yield m
    m.close()


# ---- 1. the ragged read-out kernel alone ------------------------------------------------------------------------------------
LAUNCHES = [("A", 16, [1, 2, 3, 63, 64, 65, 255, 256]), ("B", 64, [257, 512, 5, 256, 64, 1, 129, 511]), ("C", 1, [3, 5, 17, 33]),
            ("D", 2, [90])]
WINDOWS = [("content_limit0", lambda S: (1, S - 1, 0)), ("whole_row_limit_inside", lambda S: (0, S, S // 2)),
           ("content_limit_S", lambda S: (1, S - 1, S))]


def diag_rows(rows, windows):
    """rows: [probs [n_align][1][S_r]]; windows: [(lo, hi, limit)] -> per row (p [1][S_r], pos [1], prob [1], mass [1]).
    NaN sits behind every row's length in the input; the output rows must keep their fill from S_r on."""
    n, R = rows[0].shape[0], len(rows)
    S = np.asarray([r.shape[2] for r in rows], np.int32)
    probs = np.full((n, R, STRIDE), np.nan, np.float32)
    for r, x in enumerate(rows):
        probs[:, r, :S[r]] = x[:, 0, :]
    lo, hi, limit = (np.asarray([w[i] for w in windows], np.int32) for i in range(3))
    p = np.full((R, STRIDE), SENTINEL, np.float32)
    pos, prob, mass = np.full(R, -7, np.int32), np.full(R, np.nan, np.float32), np.full(R, np.nan, np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)           # noqa: E731
    lib = _lib.load()
    rc = lib.wlk_diag_nllb_align_rows(ptr(probs), n, R, STRIDE, ptr(S), ptr(lo), ptr(hi), ptr(limit), ptr(p), ptr(pos), ptr(prob),
                                      ptr(mass))
    assert rc == 0, lib.wlk_diag_last_error()
    out = []
    for r in range(R):
        assert (p[r, S[r]:] == SENTINEL).all(), f"row {r}: written at or past its length"
        assert not np.isnan(p[r, :S[r]]).any() and not np.isnan(prob[r]) and not np.isnan(mass[r]) and pos[r] != -7, f"row {r}"
        out.append((p[r:r + 1, :S[r]].copy(), pos[r:r + 1].copy(), prob[r:r + 1].copy(), mass[r:r + 1].copy()))
    return out


def launch_rows(li):
    _name, n, lens = LAUNCHES[li]
    return [AC.random_probs(n, 1, S, 200 + 16 * li + r) for r, S in enumerate(lens)]


@pytest.mark.parametrize("li", range(len(LAUNCHES)), ids=[l[0] for l in LAUNCHES])
def test_ragged_readout_kernel_against_float64(li):
    name, n, lens = LAUNCHES[li]
    rows = launch_rows(li)
    for wname, window in WINDOWS:
        wins = [window(S) for S in lens]
        for r, got in enumerate(diag_rows(rows, wins)):
            report, failures, n_exempt, _ = AC.compare("random", rows[r], *wins[r], got)
            print(f"launch {name} ({n} heads) row {r} (S = {lens[r]}) {wname} {wins[r]}: p error {report['p']['kernel_err']:.3e} "
                  f"(float32 restatement {report['p']['restatement_err']:.3e}, allowed {report['p']['allowed']:.3e}), mass error "
                  f"{report['mass']['kernel_err']:.3e} (allowed {report['mass']['allowed']:.3e}), exempt rows {n_exempt}")
            assert not failures, (name, r, wname, failures)
            assert n_exempt == 0, (name, r, wname)
            if wins[r][0] >= wins[r][1]:
                assert got[1][0] == -1 and got[2][0] == 0


def planted(base, kind):
    """-> (probs, (lo, hi, limit), the position that must win or -1); rows too short for a content window get the empty kinds"""
    S = base.shape[2]
    p = base.copy()
    lo2, hi2 = 2, S - 2
    if S < 5 or kind >= 4:
        return (p, (min(2, S), min(2, S), S // 3), -1) if kind % 2 == 0 else (p, (S, 0, 0), -1)
    mid = (lo2 + hi2) // 2
    if kind == 0:                                           # the maximum at lo
        p[:, :, lo2] = np.float32(0.75)
        return p, (lo2, hi2, 0), lo2
    if kind == 1:                                           # at hi - 1
        p[:, :, hi2 - 1] = np.float32(0.75)
        return p, (lo2, hi2, S), hi2 - 1
    if kind == 2:                                           # a larger value AT hi: outside the window, ignored
        p[:, :, mid] = np.float32(0.75)
        p[:, :, hi2] = np.float32(0.875)
        return p, (lo2, hi2, hi2), mid
    for j in {lo2, mid, hi2 - 1, hi2, 0}:                   # an exact tie: the lowest position of the window wins
        p[:, :, j] = np.float32(0.75)
    return p, (lo2, hi2, 0), lo2


@pytest.mark.parametrize("li", range(len(LAUNCHES)), ids=[l[0] for l in LAUNCHES])
def test_ragged_readout_kernel_planted_rows(li):
    """every planted kind visits every row (row r of call c holds kind (r + c) % 6), so neighbouring rows always carry
    different windows: a kernel that read row 0's window, or row 0's length, for every row fails"""
    name, _n, lens = LAUNCHES[li]
    base = launch_rows(li)
    for c in range(6):
        made = [planted(base[r], (r + c) % 6) for r in range(len(lens))]
        got = diag_rows([m[0] for m in made], [m[1] for m in made])
        if len(lens) > 1:
            assert len({m[1] for m in made}) > 1
        for r, (probs, win, winner) in enumerate(made):
            _report, failures, _exempt, _ = AC.compare("planted", probs, *win, got[r])
            assert not failures, (name, c, r, win, failures)          # (the position is the float64 reference's: no exempt row)
            if winner < 0:
                assert got[r][1][0] == -1 and got[r][2][0] == 0, (name, c, r, win)


# ---- 2. step_align against transformers ---------------------------------------------------------------------------------------
def follow_greedy_stacked(batch, prefixes, slots, atol, min_gap=0.0, leave=True):
    """A.follow_greedy for several cases at once: case i in slots[i]; all take each step together, then (leave) the cases
    leave one by one so that every smaller row count is replayed too.  -> (largest |p - p64|, row counts used)"""
    n = len(prefixes)
    srcs = [KAT[p + "src"] for p in prefixes]
    greedy = [KAT[p + "greedy"].tolist() for p in prefixes]
    steps = len(greedy[0])
    assert all(len(g) == steps for g in greedy) and steps >= n
    batch.encode(slots, srcs)
    batch.prefill(slots, [[START]] * n)
    worst, counts = 0.0, set()
    for t in range(steps):
        live = list(range(n if not leave else min(n, steps - t)))      # the last n - 1 steps lose one case each
        toks = [int(KAT[prefixes[i] + "lang"]) if t == 0 else greedy[i][t - 1] for i in live]
        _lp, ids, pos, prob, mass = batch.step_align([slots[i] for i in live], toks, 1, [1] * len(live),
                                                     [len(srcs[i]) - 1 for i in live], [0] * len(live))
        counts.add(len(live))
        for r, i in enumerate(live):
            want = KAT[prefixes[i] + "p64"][t]
            p = batch.alignment(slots[i])
            assert p.shape == (len(srcs[i]),)
            worst = max(worst, float(np.abs(p - want).max()))
            np.testing.assert_allclose(p, want, rtol=0, atol=atol, err_msg=f"{prefixes[i]} step {t}")
            if KAT[prefixes[i] + "gap"][t] > min_gap:
                assert int(pos[r]) == int(KAT[prefixes[i] + "pos"][t]), (prefixes[i], t)
                assert abs(float(prob[r]) - want[int(pos[r])]) <= atol
            assert int(ids[r, 0]) == greedy[i][t], (prefixes[i], t)
            assert abs(float(mass[r]) - want.sum()) <= atol
    return worst, counts


@pytest.mark.parametrize("slots", [[0, 1, 2, 3, 4, 5], [6, 2, 7, 0, 5, 3]], ids=["in_order", "permuted"])
def test_step_align_matches_transformers_in_six_slots(micro_hip, slots):
    batch = micro_hip.new_batch(8)
    try:
        batch.set_alignment_heads(HEADS)
        worst, counts = follow_greedy_stacked(batch, [f"c{ci}_" for ci in range(N_CASES)], slots, P_ATOL)
        print(f"six cases in slots {slots}: largest |p - p64| {worst:.3e} (bound {P_ATOL:.0e}); row counts replayed {sorted(counts)}")
        assert counts == {1, 2, 3, 4, 5, 6}
        assert batch.align_stats()["graph_captures"] == 6
    finally:
        batch.close()


def test_step_align_matches_transformers_at_the_600m_shape():
    cfg = nllb.NLLB_200_DISTILLED_600M
    model = nllb.HipNllbModel.from_hf_state_dict(cfg, A.align_gain_state_dict(cfg, int(KAT["big_seed"])), device=0, max_src=64,
                                                 max_tgt=32)
    batch = model.new_batch(8)
    try:
        batch.set_alignment_heads([tuple(h) for h in KAT["big_heads"].tolist()])
        worst, _ = follow_greedy_stacked(batch, ["big_"], [5], P_ATOL_600M, min_gap=GAP_600M, leave=False)
        print(f"600M shape in slot 5: largest |p - p64| {worst:.3e} (bound {P_ATOL_600M:.0e})")
    finally:
        batch.close()
        model.close()


# ---- 3. nothing else moves -------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("rows", [1, 3, 8])
def test_step_align_leaves_the_step_results_bit_for_bit(micro_hip, rows):
    a, b = micro_hip.new_batch(8), micro_hip.new_batch(8)
    try:
        a.set_alignment_heads(HEADS)
        slots = list(range(rows))
        srcs = [KAT[f"c{r % N_CASES}_src"][:len(KAT[f"c{r % N_CASES}_src"]) - (r // N_CASES)] for r in range(rows)]
        srcs = [np.concatenate([s[:-1], [CFG.eos_token_id]]) for s in srcs]
        S = [len(s) for s in srcs]
        for x in (a, b):
            x.encode(slots, srcs)
            x.step(slots, [START] * rows, 4)
        toks = [1991 + r for r in range(rows)]
        for step in range(4):
            lp_a, id_a, pos, prob, mass = a.step_align(slots, toks, 4, [1] * rows, [s - 1 for s in S], [s // 2 for s in S])
            lp_b, id_b = b.step(slots, toks, 4)
            assert np.array_equal(bits(lp_a), bits(lp_b)) and np.array_equal(id_a, id_b), f"step {step}"
            for r in range(rows):       # the results travel in the host-coherent block: they are the exported p's
                p = a.alignment(r)
                assert p.shape == (S[r],)
                if S[r] > 2:
                    assert pos[r] == 1 + int(np.argmax(p[1:S[r] - 1])) and prob[r] == p[pos[r]]
                else:
                    assert pos[r] == -1 and prob[r] == 0
                assert abs(mass[r] - p[S[r] // 2:].sum(dtype=np.float64)) < 1e-6
            toks = id_a[:, 0].tolist()
        lp_a, id_a = a.step(slots, toks, 4)         # the two step kinds share the caches
        lp_b, id_b = b.step(slots, toks, 4)
        assert np.array_equal(bits(lp_a), bits(lp_b)) and np.array_equal(id_a, id_b)
        assert a.align_stats() == {"align_steps": 4, "graph_captures": 1}
        assert b.align_stats() == {"align_steps": 0, "graph_captures": 0}
        a.alignment(0)                              # a plain step leaves the latest align step's p readable
    finally:
        a.close(); b.close()


def test_generate_batch_is_unchanged_with_heads_set():
    kat = H.golden_npz("nllb_batch_kat.npz")
    cases = [tuple(int(v) for v in row) for row in kat["cases"]]
    model = nllb.HipNllbModel.from_hf_state_dict(CFG, nllb.synth_state_dict(CFG, int(kat["seed"]), float(kat["eos_gain"])), device=0,
                                                 max_src=92, max_tgt=64)
    batch = model.new_batch(8)
    try:
        batch.set_alignment_heads(HEADS)
        n = len(cases)
        got = nllb.generate_batch(batch, [kat[f"src{i}"] for i in range(n)], [c[1] for c in cases], max_new_tokens=[c[2] for c in cases])
        assert got == [kat[f"gen{i}"].tolist() for i in range(n)]
        assert batch.align_stats() == {"align_steps": 0, "graph_captures": 0}
    finally:
        batch.close()
        model.close()


# ---- 4. rows are independent ---------------------------------------------------------------------------------------------------
def test_a_row_does_not_depend_on_its_neighbours(micro_hip):
    """the 20-token source in slot 4, alone and among seven neighbours of 2 .. 92 tokens: the same bits"""
    many, one = micro_hip.new_batch(8), micro_hip.new_batch(8)
    try:
        rng = np.random.default_rng(11)
        lens = [20, 3, 92, 9, 64, 33, 2, 65]
        srcs = [np.concatenate([[1990], rng.integers(4, 1900, size=n - 2), [CFG.eos_token_id]]).astype(np.int64) for n in lens]
        slot_of = [4, 6, 3, 0, 7, 1, 5, 2]                       # source i lives in slot_of[i]; the subject is source 0
        S_of = {slot_of[i]: lens[i] for i in range(8)}
        for x in (many, one):
            x.set_alignment_heads(HEADS)
        many.encode(slot_of, srcs)
        many.prefill(slot_of, [[START]] * 8)
        one.encode([4], [srcs[0]])
        one.prefill([4], [[START]])
        rows = [3, 6, 0, 4, 7, 1, 5, 2]                          # the subject is row 3 of the stacked step
        tok = 1991
        for step in range(3):
            lp8, id8, pos8, prob8, mass8 = many.step_align(rows, [tok] * 8, 4, [1] * 8, [S_of[s] - 1 for s in rows],
                                                           [S_of[s] // 3 for s in rows])
            lp1, id1, pos1, prob1, mass1 = one.step_align([4], [tok], 4, [1], [lens[0] - 1], [lens[0] // 3])
            assert np.array_equal(bits(lp8[3]), bits(lp1[0])) and np.array_equal(id8[3], id1[0]), step
            assert pos8[3] == pos1[0] and bits(prob8[3:4]) == bits(prob1) and bits(mass8[3:4]) == bits(mass1), step
            assert many.alignment(4).tobytes() == one.alignment(4).tobytes(), step
            assert pos8[rows.index(5)] == -1                     # the 2-token neighbour has no content window
            tok = int(id1[0, 0])
    finally:
        many.close(); one.close()


# ---- 5. prefill ---------------------------------------------------------------------------------------------------------------
def one_align_step(batch, slot, prompt, S):
    lp, ids, pos, prob, mass = batch.step_align([slot], [prompt[-1]], 1, [1], [S - 1], [0])
    return int(ids[0, 0]), int(pos[0]), batch.alignment(slot)


@pytest.mark.parametrize("committed", [0, 1, 5, 11])
def test_prefill_equals_token_by_token_steps_and_the_session(micro_hip, committed):
    prefix = "c4_"
    src, lang, greedy = KAT[prefix + "src"], int(KAT[prefix + "lang"]), KAT[prefix + "greedy"].tolist()
    S = len(src)
    prompt = [START, lang] + greedy[:committed]
    batch, sess = micro_hip.new_batch(3), micro_hip.new_session(1)
    try:
        batch.set_alignment_heads(HEADS)
        sess.set_alignment_heads(HEADS)
        batch.encode([2, 0], [src, src])
        batch.prefill([2], [prompt[:-1]])                                   # slot 2: one stacked pass over the prompt
        for tok in prompt[:-1]:                                              # slot 0: the same prompt token by token
            batch.step([0], [tok], 1)
        y_pre, a_pre, p_pre = one_align_step(batch, 2, prompt, S)
        y_tok, a_tok, p_tok = one_align_step(batch, 0, prompt, S)
        sess.encode(src)
        sess.decode(np.asarray([prompt[:-1]], np.int64), first=True)
        _lp, ids, pos, _prob, _mass = sess.step_align([prompt[-1]], 1, 1, S - 1, 0)
        p_sess = sess.alignment()[0]
        want = KAT[prefix + "p64"][committed]
        print(f"{committed} committed ids: |prefill - steps| {float(np.abs(p_pre - p_tok).max()):.3e}, |prefill - session| "
              f"{float(np.abs(p_pre - p_sess).max()):.3e}, |prefill - p64| {float(np.abs(p_pre - want).max()):.3e}")
        assert (y_pre, a_pre) == (y_tok, a_tok) == (int(ids[0, 0]), int(pos[0])) == (greedy[committed], int(KAT[prefix + "pos"][committed]))
        for p in (p_pre, p_tok, p_sess):
            np.testing.assert_allclose(p, want, rtol=0, atol=P_ATOL)
    finally:
        batch.close(); sess.close()


def test_prefill_of_four_slots_in_one_call_equals_four_calls(micro_hip):
    cases, n_committed = [0, 2, 4, 5], [0, 1, 5, 11]                       # prompt[:-1] of 1, 2, 6 and 12 tokens
    srcs = [KAT[f"c{ci}_src"] for ci in cases]
    prompts = [[START, int(KAT[f"c{ci}_lang"])] + KAT[f"c{ci}_greedy"].tolist()[:c] for ci, c in zip(cases, n_committed)]
    assert [len(p) - 1 for p in prompts] == [1, 2, 6, 12]
    together, apart = micro_hip.new_batch(4), micro_hip.new_batch(4)
    try:
        for x in (together, apart):
            x.set_alignment_heads(HEADS)
            x.encode([3, 1, 0, 2], srcs)
        together.prefill([3, 1, 0, 2], [p[:-1] for p in prompts])
        for slot, p in zip([3, 1, 0, 2], prompts):
            apart.prefill([slot], [p[:-1]])
        for slot, p, src, ci, c in zip([3, 1, 0, 2], prompts, srcs, cases, n_committed):
            got, want = one_align_step(together, slot, p, len(src)), one_align_step(apart, slot, p, len(src))
            print(f"case {ci}, {len(p) - 1} prompt rows: |one call - own call| {float(np.abs(got[2] - want[2]).max()):.3e}")
            assert got[:2] == want[:2] == (KAT[f"c{ci}_greedy"].tolist()[c], int(KAT[f"c{ci}_pos"][c]))
            np.testing.assert_allclose(got[2], KAT[f"c{ci}_p64"][c], rtol=0, atol=P_ATOL)
            np.testing.assert_allclose(want[2], KAT[f"c{ci}_p64"][c], rtol=0, atol=P_ATOL)
    finally:
        together.close(); apart.close()


# ---- 6. the loop ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_slots", [8, 3])
def test_generate_alignatt_batch_returns_the_stored_outcomes(micro_hip, n_slots):
    reqs, want = B.all_requests(KAT, A.settings_of)
    assert len(reqs) == 78
    batch = micro_hip.new_batch(n_slots)
    row_counts = set()
    step_align = batch.step_align
    batch.step_align = lambda slots, *a: (row_counts.add(len(slots)), step_align(slots, *a))[1]
    try:
        batch.set_alignment_heads(HEADS)
        got = nllb.generate_alignatt_batch(batch, reqs)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, f"request {i}: {reqs[i][2:]}"
        sess = micro_hip.new_session(1)                   # ... and every setting is generate_alignatt's answer on a session
        try:
            sess.set_alignment_heads(HEADS)
            for i, (src, lang, committed, n_acc, thr, final, max_new) in enumerate(reqs):
                assert got[i] == nllb.generate_alignatt(sess, src, lang, committed=committed, n_accessible=n_acc, threshold=thr,
                                                        final=final, max_new_tokens=max_new), i
        finally:
            sess.close()
        stats = batch.align_stats()
        print(f"{n_slots} slots: {stats['align_steps']} align steps for 78 updates, {stats['graph_captures']} recordings, row counts "
              f"{sorted(row_counts)}")
        assert 0 < stats["graph_captures"] <= len(row_counts) <= n_slots
    finally:
        batch.close()


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------
def raises(code, fn, *a):
    with pytest.raises(WlkError) as e:
        fn(*a)
    assert err_code(e) == code, (fn.__name__, a, str(e.value))


def test_errors_leave_the_batch_usable():
    model = nllb.HipNllbModel.from_hf_state_dict(CFG, A.align_gain_state_dict(CFG, 0), device=0, max_src=92, max_tgt=8)
    batch = model.new_batch(3)
    try:
        for bad in ([(2, 0)], [(0, 2)], [(-1, 0)], [(0, 0), (0, 0)], [(0, 0)] * 65):
            raises(WLK_ERR_ARG, batch.set_alignment_heads, bad)
        src, lang, greedy = KAT["c2_src"], int(KAT["c2_lang"]), KAT["c2_greedy"].tolist()
        S = len(src)
        batch.encode([0, 1], [src, src])
        batch.prefill([0], [[START]])
        raises(WLK_ERR_STATE, batch.step_align, [0], [lang], 1, [1], [S - 1], [0])            # before heads are set
        raises(WLK_ERR_STATE, batch.alignment, 0)
        batch.set_alignment_heads(HEADS)
        raises(WLK_ERR_STATE, batch.step_align, [1], [lang], 1, [1], [S - 1], [0])            # a slot without a prompt
        raises(WLK_ERR_STATE, batch.step_align, [2], [lang], 1, [1], [S - 1], [0])            # a slot that is not encoded
        for lo, hi, limit in [(-1, S - 1, 0), (1, S + 1, 0), (1, S - 1, -1), (1, S - 1, S + 1)]:
            raises(WLK_ERR_ARG, batch.step_align, [0], [lang], 1, [lo], [hi], [limit])
        for k in (0, 9):
            raises(WLK_ERR_ARG, batch.step_align, [0], [lang], k, [1], [S - 1], [0])
        raises(WLK_ERR_ARG, batch.step_align, [0, 0], [lang, lang], 1, [1, 1], [S - 1] * 2, [0, 0])
        raises(WLK_ERR_ARG, batch.step_align, [0], [CFG.pad_token_id], 1, [1], [S - 1], [0])
        raises(WLK_ERR_STATE, batch.prefill, [0], [[START]])                                   # already holds target tokens
        raises(WLK_ERR_STATE, batch.prefill, [2], [[START]])                                   # not encoded
        raises(WLK_ERR_CAPACITY, batch.prefill, [1], [[START] + [lang] * 7])                   # 8 > max_tgt - 1
        raises(WLK_ERR_ARG, batch.prefill, [1], [[START, 99999]])
        raises(WLK_ERR_ARG, batch.prefill, [1], [[START, CFG.pad_token_id]])
        raises(WLK_ERR_ARG, batch.prefill, [1, 1], [[START], [START]])
        raises(WLK_ERR_ARG, batch.prefill, [1], [[]])
        # after all that: slot 0 takes its step, slot 1 its prefill, and both give the fixture's first position
        batch.prefill([1], [[START]])
        _lp, ids, pos, _prob, _mass = batch.step_align([1, 0], [lang, lang], 1, [1, 1], [S - 1] * 2, [0, S])
        assert ids[:, 0].tolist() == [greedy[0]] * 2 and pos.tolist() == [int(KAT["c2_pos"][0])] * 2
        np.testing.assert_allclose(batch.alignment(0), KAT["c2_p64"][0], rtol=0, atol=P_ATOL)
        batch.step([1], [greedy[0]], 1)
        raises(WLK_ERR_STATE, batch.logits, 0)                   # slot 0 was not in the latest step
        assert batch.alignment(0).shape == (S,)                                                # ... its p of the align step stays
        batch.release(0)
        raises(WLK_ERR_STATE, batch.alignment, 0)
        # the context stop, on this tight max_tgt = 8: generate_alignatt's answer on a session of the same model
        sess = model.new_session(1)
        try:
            sess.set_alignment_heads(HEADS)
            want = nllb.generate_alignatt(sess, src, lang, n_accessible=S, threshold=0, final=True, max_new_tokens=199)
        finally:
            sess.close()
        batch.release(1)
        got = nllb.generate_alignatt_batch(batch, [(src, lang, [], S, 0, True, 199), (src, lang, greedy[:6], S, 0, True, 199),
                                                   (src, lang, greedy[:7], S, 0, True, 199)])
        assert got[0] == want and want[2] == "context" and len(want[0]) == 7
        assert got[1] == ([greedy[6]], [int(KAT["c2_pos"][6])], "context") and got[2] == ([], [], "context")
        batch.set_alignment_heads([])                                                           # switched off again
        batch.encode([0], [src])
        batch.prefill([0], [[START]])
        raises(WLK_ERR_STATE, batch.step_align, [0], [lang], 1, [1], [S - 1], [0])
    finally:
        batch.close()
        model.close()


# ---- 8. serving on the device -------------------------------------------------------------------------------------------------
def words(spec, t0=0.0):
    return [ASRToken(start=round(t0 + 0.4 * i, 2), end=round(t0 + 0.4 * i + 0.4, 2), text=" " + w) for i, w in enumerate(spec.split())]


def stream_sentence(tm, barrier=None):
    """A.SENTENCE word by word with a two-word tail (tests/nllb_align_standin.py stream_twelve_words' stream) -> every call's texts"""
    toks = words(A.SENTENCE)
    now = [0.0]
    tr = tm.new_session("eng_Latn", "fra_Latn")
    tr._clock = lambda: now[0]
    log = []
    try:
        for i, w in enumerate(toks[:-1]):
            now[0] += 1.0
            tr.insert_tokens([w, A.HypothesisTail(" ".join(t.text.strip() for t in toks[i + 1:i + 3]))])
            if barrier is not None:
                barrier.wait(60)                                  # the sessions' updates fall on the same tick
            log.append(tr.process())
        tr.insert_tokens(toks[-1:])
        log.append(tr.process())
        return [(None if new is None else (new.start, new.end, new.text), buf.text) for new, buf in log], tr.updates + tr.finals
    finally:
        tr.close()


def test_eight_stacked_sessions_on_the_device(micro_hip, monkeypatch):
    monkeypatch.delenv("WLK_NLLB_STACK", raising=False)
    kw = dict(policy="alignatt", threshold=2, hypothesis_tail=True, max_new_tokens=24)
    want, n_passes = stream_sentence(T.HipNllbTranslationModel(micro_hip, B.HashTokenizer(CFG.eos_token_id), **kw))
    assert want[-1][0] is not None and n_passes > 1
    tm = T.HipNllbTranslationModel(micro_hip, B.HashTokenizer(CFG.eos_token_id), stack=8, **kw)
    got, errors = [None] * 8, []
    barrier = threading.Barrier(8)

    def work(i):
        try:
            got[i] = stream_sentence(tm, barrier)
        except BaseException as e:       # noqa: BLE001 - reported below
            errors.append(e)
            barrier.abort()

    try:
        threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(8)]
        for th in threads:
            th.start()
        for th in threads:
            th.join(120)
        assert not any(th.is_alive() for th in threads), "a session thread hangs"
        assert not errors, errors
        assert all(g == (want, n_passes) for g in got)
        stats = tm.batch.align_stats()
        print(f"8 sessions x {n_passes} updates: {tm.stacker.passes} stacked passes, {stats['align_steps']} align steps, "
              f"{stats['graph_captures']} recordings")
        assert tm.stacker.sentences == 8 * n_passes and 0 < tm.stacker.passes < tm.stacker.sentences
    finally:
        tm.close()
