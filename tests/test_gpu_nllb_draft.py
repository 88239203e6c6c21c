"""NLLB draft verification on the GPU: wlk_nllb_batch_verify, its two kernels and the serving path.

1.  the pick kernel alone (wlk_diag_nllb_verify_pick) against np.argmax and wlk_diag_topk(k = 1), exactly;
2.  accepted / next token of planted wrong tokens (positions 0, 1, 63, 64, 65, last) and of whole truths;
3.  stepping on after every such verify reproduces the fixture's ids (= nllb.generate on a session);
4.  the rows a rejected draft leaves behind position 2 + k change nothing (bitwise, twin batches);
5.  against wlk_nllb_batch_prefill: bitwise after a fully accepted draft, within LOGIT_ATOL after a rejected one;
6.  1, 2, 3, 5, 8 slots per call in shuffled order == each slot alone, a slot in the middle of a decode is left alone;
7.  more rows than one read-out chunk (128), one slot's rows on both sides of the boundary;
8.  refusals: the documented code, nothing launched, the slots go on to a twin's bits;
9.  the 600M shape;
10. generate_batch(drafts) and four serving threads with draft=True.

Truths come from tests/golden/nllb_draft_kat.npz: every compared pick keeps a float64 gap >= 2e-3 = twice LOGIT_ATOL
(nllb_draft_cases.py), so no test allows for ties.  The micro model has max_tgt = 80."""
import ctypes as C
import threading

import numpy as np
import pytest

import nllb_draft_cases as DC
from test_translation import WordTokenizer
from whisperlivekit_amd import _lib, nllb
from whisperlivekit_amd import translation as T

pytestmark = pytest.mark.gpu

FX = DC.Fixture()
CFG = DC.CFG
EOS, START = CFG.eos_token_id, CFG.decoder_start_token_id
LOGIT_ATOL = 1e-3                      # tests/test_nllb.py / test_nllb_batch.py: the project's stacked-versus-solo allowance
V_NLLB = 256206
WLK_ERR_ARG, WLK_ERR_STATE, WLK_ERR_CAPACITY = -1, -3, -4
LONG = FX.long_case()


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- 1. the pick kernel --------------------------------------------------------------------------------------------------------
def diag_pick(x, targets):
    x = np.ascontiguousarray(x, np.float32)
    R, V = x.shape
    t = np.ascontiguousarray(targets, np.int32)
    picks, match = np.full(R, -7, np.int32), np.full(R, -7, np.int32)
    lib = _lib.load()
    rc = lib.wlk_diag_nllb_verify_pick(ptr(x), R, V, ptr(t), ptr(picks), ptr(match))
    assert rc == 0, lib.wlk_diag_last_error()
    return picks, match


def diag_top1(x):
    x = np.ascontiguousarray(x, np.float32)
    lib = _lib.load()
    out = []
    for r0 in range(0, x.shape[0], 64):                                  # wlk_diag_topk takes 64 rows a call
        part = np.ascontiguousarray(x[r0:r0 + 64])
        vals, ids = np.empty((part.shape[0], 1), np.float32), np.empty((part.shape[0], 1), np.int32)
        assert lib.wlk_diag_topk(ptr(part), part.shape[0], part.shape[1], 1, 0, ptr(vals), ptr(ids)) == 0, lib.wlk_diag_last_error()
        out.append(ids[:, 0])
    return np.concatenate(out)


def slice_bounds(V):
    per = (((V + 31) // 32) + 1) & ~1                                    # nllb_verify_pick_rows_kernel's partition
    return per, [(s * per, min(V, s * per + per)) for s in range(32) if s * per < V]


PLACEMENTS = ("random", "max_at_0", "max_at_end", "tie_across_slices", "tie_in_one_wave", "minus_inf_but_one", "all_equal",
              "all_negative")


def planted(V, rows, placement, rng):
    x = rng.standard_normal((rows, V)).astype(np.float32)
    per, bounds = slice_bounds(V)
    for r in range(rows):
        if placement == "max_at_0":
            x[r, 0] = 9.0
        elif placement == "max_at_end":
            x[r, V - 1] = 9.0
        elif placement == "tie_across_slices":
            a = bounds[r % len(bounds)][0] + (1 if V > 2 * per else 0)
            b = bounds[-1][1] - 1 - (r % 2)
            x[r, [min(a, b), max(a, b)]] = 9.0
            if len(bounds) > 2:
                x[r, bounds[len(bounds) // 2][0]] = 9.0
        elif placement == "tie_in_one_wave":
            lo, hi = bounds[(3 * r) % len(bounds)]
            a = lo + (5 * r) % max(1, min(100, hi - lo - 3))
            x[r, [a, min(a + 3, hi - 1)]] = 9.0                          # pairs a / 2 and (a + 3) / 2: lanes of one wave
        elif placement == "minus_inf_but_one":
            keep = (r * 7919 + V // 3) % V
            v = x[r, keep]
            x[r] = -np.inf
            x[r, keep] = v
        elif placement == "all_equal":
            x[r] = np.float32(0.25 * (r + 1))
        elif placement == "all_negative":
            x[r] = -np.abs(x[r]) - 1.0
    return x


@pytest.mark.parametrize("V,rows", [(7, 1), (7, 3), (2003, 1), (2003, 3), (2003, 70), (V_NLLB, 1), (V_NLLB, 3)])
def test_pick_kernel_is_the_exact_arg_max(V, rows):
    rng = np.random.default_rng(V + rows)
    for placement in PLACEMENTS:
        x = planted(V, rows, placement, rng)
        want = np.argmax(x, axis=1).astype(np.int32)                      # the first maximum: the lowest id on a tie
        targets = want.copy()
        targets[::2] = (targets[::2] + 1) % V                             # every other row's target is NOT the pick
        picks, match = diag_pick(x, targets)
        assert picks.tolist() == want.tolist(), (V, rows, placement)
        assert match.tolist() == (want == targets).astype(np.int32).tolist(), (V, rows, placement)
        assert diag_top1(x).tolist() == want.tolist(), (V, rows, placement)


def test_pick_diag_refuses_bad_shapes():
    lib = _lib.load()
    x, t, o = np.zeros((1, 8), np.float32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    assert lib.wlk_diag_nllb_verify_pick(ptr(x), 0, 8, ptr(t), ptr(o), ptr(o)) == WLK_ERR_ARG
    assert lib.wlk_diag_nllb_verify_pick(ptr(x), 129, 8, ptr(t), ptr(o), ptr(o)) == WLK_ERR_ARG
    assert lib.wlk_diag_nllb_verify_pick(ptr(x), 1, 0, ptr(t), ptr(o), ptr(o)) == WLK_ERR_ARG
    assert lib.wlk_diag_nllb_verify_pick(ptr(x), 1, 8, None, ptr(o), ptr(o)) == WLK_ERR_ARG


# ---- the micro model -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def micro_hip():
    m = nllb.HipNllbModel.from_hf_state_dict(CFG, FX.micro_weights(), device=0, max_src=92, max_tgt=DC.MAX_TGT)
    yield m
    m.close()


def draft_of(i):
    return nllb.clamp_draft(FX.gen[i], FX.limit[i], DC.MAX_TGT, EOS)


def tokens_of(i, wrong_at=None):
    """[start, language] + the clamped draft of truth i, a wrong token planted at draft position wrong_at"""
    d = draft_of(i)
    if wrong_at is not None:
        d[wrong_at] = 7 if d[wrong_at] != 7 else 8
    return FX.gen[i][:2] + d


def expected(i, wrong_at=None):
    k = len(draft_of(i)) if wrong_at is None else wrong_at
    return k, FX.gen[i][2 + k]


def step_to_the_end(batch, slot, i, out):
    """generate_batch's loop for one sentence from `out` on"""
    out = list(out)
    while out[-1] != EOS and len(out) < 1 + FX.limit[i]:
        out.append(int(batch.step([slot], [out[-1]], 1)[1][0, 0]))
    return out


_ALONE = {}


def verified_alone(model, i, wrong_at=None):
    key = (i, wrong_at)
    if key not in _ALONE:
        batch = model.new_batch(1)
        try:
            batch.encode([0], [FX.src[i]])
            k, nxt = batch.verify([0], [tokens_of(i, wrong_at)])
            _ALONE[key] = (int(k[0]), int(nxt[0]))
        finally:
            batch.close()
    return _ALONE[key]


def wrong_positions(i):
    n_d = len(draft_of(i))
    at = [None, 0, 1, n_d - 1]
    if i == LONG:
        at += [63, 64, 65]
    return [a for a in at if a is None or a < n_d]


def test_session_generate_gives_the_fixture(micro_hip):
    sess = micro_hip.new_session(1)
    try:
        for i in range(FX.n):
            assert nllb.generate(sess, FX.src[i], FX.lang[i], max_new_tokens=FX.limit[i]) == FX.gen[i], i
    finally:
        sess.close()


# ---- 2. + 3. accept and continuation ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(FX.n))
def test_accepted_prefix_next_token_and_continuation(micro_hip, i):
    if not draft_of(i):
        pytest.fail(f"truth {i} of the fixture leaves no draft")
    batch = micro_hip.new_batch(1)
    try:
        for at in wrong_positions(i):
            batch.encode([0], [FX.src[i]])
            before = batch.verify_stats()
            k, nxt = batch.verify([0], [tokens_of(i, at)])
            assert (int(k[0]), int(nxt[0])) == expected(i, at), (i, at)
            after = batch.verify_stats()
            assert after["passes"] == before["passes"] + 1 and after["draft_tokens"] == before["draft_tokens"] + len(draft_of(i))
            assert after["accepted_tokens"] == before["accepted_tokens"] + int(k[0])
            with pytest.raises(_lib.WlkError):
                batch.logits(0)                                           # as after a prefill: no logits row
            out = FX.gen[i][:2 + int(k[0])] + [int(nxt[0])]
            assert step_to_the_end(batch, 0, i, out) == FX.gen[i], (i, at)
            batch.release(0)
    finally:
        batch.close()


# ---- 4. stale rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,k", [(LONG, 3), (LONG, 40), (LONG, 64)])
def test_rows_of_a_rejected_draft_change_nothing(micro_hip, i, k):
    d = draft_of(i)
    rng = np.random.default_rng(k)
    tails = []
    for _ in range(2):
        tail = rng.integers(4, 1900, size=len(d) - k).tolist()
        tail[0] = 9 if d[k] != 9 else 10                                  # not the truth's token: the draft is cut at k
        tails.append(tail)
    assert tails[0] != tails[1]
    a, b = micro_hip.new_batch(1), micro_hip.new_batch(1)
    try:
        got = []
        for batch, tail in zip((a, b), tails):
            batch.encode([0], [FX.src[i]])
            kk, nxt = batch.verify([0], [FX.gen[i][:2] + d[:k] + tail])
            got.append((int(kk[0]), int(nxt[0])))
        assert got[0] == got[1] == (k, FX.gen[i][2 + k])
        tok = got[0][1]
        for step in range(4):
            ids = [int(batch.step([0], [tok], 1)[1][0, 0]) for batch in (a, b)]
            assert a.logits(0).tobytes() == b.logits(0).tobytes(), (k, step)
            assert ids[0] == ids[1] == FX.gen[i][3 + k + step]
            tok = ids[0]
    finally:
        a.close(); b.close()


# ---- 5. against the prefill --------------------------------------------------------------------------------------------------------
def test_fully_accepted_draft_leaves_the_prefills_bits(micro_hip):
    group = [LONG, 1, 4, 6]
    a, b = micro_hip.new_batch(4), micro_hip.new_batch(4)
    try:
        slots = [2, 0, 3, 1]
        lists = [tokens_of(i) for i in group]
        for batch in (a, b):
            batch.encode(slots, [FX.src[i] for i in group])
        k, nxt = a.verify(slots, lists)
        assert k.tolist() == [len(draft_of(i)) for i in group]
        b.prefill(slots, lists)                                           # the same chain over the same table
        a.step(slots, nxt.tolist(), 1)
        b.step(slots, nxt.tolist(), 1)
        for s in slots:
            assert a.logits(s).tobytes() == b.logits(s).tobytes(), s
    finally:
        a.close(); b.close()


def test_rejected_draft_against_a_prefill_of_the_accepted_prefix(micro_hip):
    worst = 0.0
    a, b = micro_hip.new_batch(1), micro_hip.new_batch(1)
    try:
        for i, at in [(LONG, 0), (LONG, 30), (LONG, 65), (2, 5), (9, 10)]:
            for batch in (a, b):
                batch.encode([0], [FX.src[i]])
            k, nxt = a.verify([0], [tokens_of(i, at)])
            assert int(k[0]) == at
            b.prefill([0], [FX.gen[i][:2 + at]])
            ia = int(a.step([0], [int(nxt[0])], 1)[1][0, 0])
            ib = int(b.step([0], [int(nxt[0])], 1)[1][0, 0])
            diff = float(np.abs(a.logits(0) - b.logits(0)).max())
            worst = max(worst, diff)
            print(f"truth {i}, draft cut at {at}: |verify - prefill| of the next step's logits {diff:.3g}")
            assert ia == ib == FX.gen[i][3 + at]
            np.testing.assert_allclose(a.logits(0), b.logits(0), rtol=0, atol=LOGIT_ATOL)
            a.release(0); b.release(0)
        print(f"worst difference {worst:.3g}")
    finally:
        a.close(); b.close()


# ---- 6. several slots ----------------------------------------------------------------------------------------------------------------
BYSTANDER = 7                          # a truth of 41 tokens, none of MIX
MIX = [(LONG, 64), (1, None), (2, 0), (4, 1), (9, None), (10, 7), (6, 2), (5, 2)]     # (truth, wrong position): different P and k


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
def test_several_slots_per_call_equal_each_slot_alone(micro_hip, n):
    rng = np.random.default_rng(n)
    members = [MIX[j] for j in rng.permutation(len(MIX))[:n]]
    slots = rng.permutation(8)[:n].tolist()                               # shuffled slot order
    batch = micro_hip.new_batch(8)
    try:
        bystander = next((s for s in range(8) if s not in slots), None)
        by_out = None
        if bystander is not None:                                         # a slot in the middle of its decode, not named below
            batch.encode([bystander], [FX.src[BYSTANDER]])
            by_out = [START]
            for _ in range(4):
                best = int(batch.step([bystander], [by_out[-1]], 1)[1][0, 0])
                by_out.append(FX.lang[BYSTANDER] if len(by_out) == 1 else best)
        batch.encode(slots, [FX.src[i] for i, _at in members])
        k, nxt = batch.verify(slots, [tokens_of(i, at) for i, at in members])
        for r, (i, at) in enumerate(members):
            assert (int(k[r]), int(nxt[r])) == verified_alone(micro_hip, i, at) == expected(i, at), (n, i, at)
        for r, (i, at) in enumerate(members):
            assert step_to_the_end(batch, slots[r], i, FX.gen[i][:2 + int(k[r])] + [int(nxt[r])]) == FX.gen[i]
        if bystander is not None:
            assert step_to_the_end(batch, bystander, BYSTANDER, by_out) == FX.gen[BYSTANDER]
    finally:
        batch.close()


# ---- 7. chunks -------------------------------------------------------------------------------------------------------------------------
def test_more_rows_than_one_read_out_chunk(micro_hip):
    members = [(LONG, 65), (9, None), (LONG, None), (LONG, 1), (2, None)]
    lists = [tokens_of(i, at) for i, at in members]
    start = np.cumsum([0] + [len(t) for t in lists])
    assert start[-1] > 2 * 128 and any(start[j] < 128 < start[j + 1] for j in range(len(lists)))      # a slot straddles row 128
    assert any(start[j] < 256 < start[j + 1] for j in range(len(lists)))
    batch = micro_hip.new_batch(8)
    try:
        slots = [4, 1, 6, 0, 3]
        batch.encode(slots, [FX.src[i] for i, _at in members])
        k, nxt = batch.verify(slots, lists)
        for r, (i, at) in enumerate(members):
            assert (int(k[r]), int(nxt[r])) == verified_alone(micro_hip, i, at) == expected(i, at), (i, at)
        for r, (i, at) in enumerate(members):
            assert step_to_the_end(batch, slots[r], i, FX.gen[i][:2 + int(k[r])] + [int(nxt[r])]) == FX.gen[i]
    finally:
        batch.close()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------
def raw_verify(batch, slots, lists, n=None, null=None):
    lib = _lib.load()
    sl = np.ascontiguousarray(slots, np.int32)
    off = np.zeros(len(lists) + 1, np.int32)
    off[1:] = np.cumsum([len(t) for t in lists])
    ids = np.ascontiguousarray(np.concatenate([np.asarray(t, np.int64) for t in lists]) if lists else np.zeros(1, np.int64))
    acc, nxt = np.full(8, -9, np.int32), np.full(8, -9, np.int64)
    args = [ptr(sl), ptr(ids), ptr(off), len(lists) if n is None else n, ptr(acc), ptr(nxt)]
    if null is not None:
        args[null] = None
    rc = lib.wlk_nllb_batch_verify(batch._h, *args)
    return rc, acc, nxt


def test_refusals_launch_nothing_and_leave_the_slots_usable(micro_hip):
    a, twin = micro_hip.new_batch(3), micro_hip.new_batch(3)
    try:
        for batch in (a, twin):
            batch.encode([0, 1], [FX.src[1], FX.src[2]])
        a.verify([1], [tokens_of(2)])                                     # (allocates the verify buffers; slot 1 now holds tokens)
        twin.verify([1], [tokens_of(2)])
        stats = a.verify_stats()
        good = tokens_of(1)
        cases = [
            ("slot not encoded", [2], [good], None, None, WLK_ERR_STATE),
            ("slot already holding tokens", [1], [good], None, None, WLK_ERR_STATE),
            ("a slot named twice", [0, 0], [good, good], None, None, WLK_ERR_ARG),
            ("slot out of range", [3], [good], None, None, WLK_ERR_ARG),
            ("P < 2", [0], [good[:1]], None, None, WLK_ERR_ARG),
            ("P > max_tgt - 1", [0], [good[:2] + [20] * (DC.MAX_TGT - 2)], None, None, WLK_ERR_CAPACITY),
            ("id out of range", [0], [good[:3] + [CFG.vocab_size]], None, None, WLK_ERR_ARG),
            ("negative id", [0], [good[:3] + [-1]], None, None, WLK_ERR_ARG),
            ("padding id", [0], [good[:3] + [CFG.pad_token_id]], None, None, WLK_ERR_ARG),
            ("n = 0", [0], [good], 0, None, WLK_ERR_ARG),
            ("n > n_slots", [0, 2, 1, 0], [good] * 4, None, None, WLK_ERR_ARG),
        ] + [(f"NULL argument {j}", [0], [good], None, j, WLK_ERR_ARG) for j in (0, 1, 2, 4, 5)]
        for name, slots, lists, n, null, code in cases:
            rc, acc, nxt = raw_verify(a, slots, lists, n, null)
            assert rc == code, (name, rc, _lib.load().wlk_last_error())
            assert a.verify_stats() == stats, name                        # nothing ran
            assert (acc == -9).all() and (nxt == -9).all(), name
        assert _lib.load().wlk_nllb_batch_verify(None, None, None, None, 1, None, None) == WLK_ERR_ARG
        # the slots go on as if nothing had been asked: slot 0 verifies, slot 1 steps - bit for bit a twin that was never refused
        for batch in (a, twin):
            k, nxt = batch.verify([0], [tokens_of(1, 1)])
            assert (int(k[0]), int(nxt[0])) == expected(1, 1)
            batch.step([0, 1], [int(nxt[0]), expected(2)[1]], 1)
        for s in (0, 1):
            assert a.logits(s).tobytes() == twin.logits(s).tobytes(), s
        assert a.verify_stats() == twin.verify_stats()
    finally:
        a.close(); twin.close()


def test_a_batch_that_never_verifies_reports_zero(micro_hip):
    batch = micro_hip.new_batch(2)
    try:
        assert batch.verify_stats() == {"passes": 0, "draft_tokens": 0, "accepted_tokens": 0}
        assert nllb.generate_batch(batch, [FX.src[1]], FX.lang[1], max_new_tokens=FX.limit[1]) == [FX.gen[1]]
        assert batch.verify_stats()["passes"] == 0
    finally:
        batch.close()


# ---- 9. the 600M shape -----------------------------------------------------------------------------------------------------------------
def test_600m_shape_accepts_up_to_the_wrong_token():
    b = FX.big
    cfg = DC.BIG_CFG
    model = nllb.HipNllbModel.from_hf_state_dict(cfg, nllb.synth_state_dict(cfg, b["seed"]), device=0, max_src=DC.BIG_MAX_SRC,
                                                 max_tgt=DC.BIG_MAX_TGT)
    batch = model.new_batch(1)
    try:
        d = nllb.clamp_draft(b["gen"], b["limit"], DC.BIG_MAX_TGT, cfg.eos_token_id)
        assert len(d) >= 8
        d[5] = 1234 if d[5] != 1234 else 1235
        batch.encode([0], [b["src"]])
        k, nxt = batch.verify([0], [b["gen"][:2] + d])
        assert (int(k[0]), int(nxt[0])) == (5, b["gen"][2 + 5])            # the stepwise token at that position
        out = b["gen"][:2 + 5] + [int(nxt[0])]
        while out[-1] != cfg.eos_token_id and len(out) < 1 + b["limit"]:
            out.append(int(batch.step([0], [out[-1]], 1)[1][0, 0]))
        assert out == b["gen"]
    finally:
        batch.close()
        model.close()


# ---- 10. end to end --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_slots", [8, 3])
def test_generate_batch_with_drafts_gives_the_fixture(micro_hip, n_slots):
    idx = list(range(FX.n))
    drafts = []
    for i in idx:
        n_d = len(draft_of(i))
        d = list(FX.gen[i])
        if i % 3 == 1:
            d[2 + (n_d // 2)] = 7 if d[2 + (n_d // 2)] != 7 else 8
        drafts.append(None if i % 3 == 2 else d)
    batch = micro_hip.new_batch(n_slots)
    try:
        got = nllb.generate_batch(batch, [FX.src[i] for i in idx], [FX.lang[i] for i in idx], max_new_tokens=[FX.limit[i] for i in idx],
                                  drafts=drafts)
        assert got == FX.gen
        stats = batch.verify_stats()
        assert stats["passes"] >= 1 and 0 < stats["accepted_tokens"] < stats["draft_tokens"]
    finally:
        batch.close()


def test_four_serving_threads_with_drafts_give_the_draft_off_texts(micro_hip, monkeypatch):
    monkeypatch.delenv("WLK_NLLB_DRAFT", raising=False)
    runs = [(DC.SCREENED_SEEDS[i], DC.SCREENED_TARGETS[i % 2]) for i in range(4)]
    off = T.HipNllbTranslationModel(micro_hip, WordTokenizer(), max_new_tokens=DC.SCREENED_LIMIT, stack=4, draft=False)
    try:
        want = [DC.drive_script(off, DC.growing_script(seed), target)[0] for seed, target in runs]
        assert off.batch.verify_stats()["passes"] == 0
    finally:
        off.close()
    on = T.HipNllbTranslationModel(micro_hip, WordTokenizer(), max_new_tokens=DC.SCREENED_LIMIT, stack=4, draft=True)
    try:
        got, errors = [None] * 4, []

        def work(j):
            try:
                got[j] = DC.drive_script(on, DC.growing_script(runs[j][0]), runs[j][1])[0]
            except BaseException as e:       # noqa: BLE001 - reported below
                errors.append(e)

        threads = [threading.Thread(target=work, args=(j,), daemon=True) for j in range(4)]
        for th in threads:
            th.start()
        for th in threads:
            th.join(120)
        assert not any(th.is_alive() for th in threads), "a session thread hangs"
        assert not errors, errors
        assert got == want
        stats = on.batch.verify_stats()
        print(f"four sessions: {stats}")
        assert stats["passes"] > 0 and stats["accepted_tokens"] > 0
    finally:
        on.close()
