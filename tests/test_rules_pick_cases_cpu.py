"""The designed cases of tests/rules_pick_cases.py hold what tests/test_gpu_rules_pick.py relies on (no GPU): float64 sees no
near-tie in them that was not planted, every margin pair flips the winner, every border case has the forbidden token on top
and an allowed winner, `history_state` is the host's `_pick_state`, and the two diagnostic entries refuse bad arguments
before they touch a device."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import rules_pick_cases as RC
import rules_topk_reference as REF
import window_burst_cases as WB
import window_group_cases as WG
from whisperlivekit_amd import _lib, transcribe as TR

WLK_ERR_ARG = -1


def winner(c, mask=None):
    lp, ids = REF.rules_topk_reference(c["logits"][None], c["mask"] if mask is None else mask, [c["state"]], 1)
    return int(ids[0, 0]), float(lp[0, 0])


def test_no_case_has_a_near_tie_that_was_not_planted():
    cases = RC.single_cases()
    assert {c["family"] for c in cases} == set(RC.FAMILIES)
    assert {c["V"] for c in cases} == set(RC.SIZES)
    assert sum(c["family"] == "margin" for c in cases) == 2 * len(RC.MARGINS) * len(RC.SCALES) * len(RC.SIZES)
    for c in cases:
        x, st = c["logits"][None], [c["state"]]
        eps = 1e-3 if c["family"] == "ties" else REF.NEAR_TIE
        assert not REF.unplanted_near_ties(x, c["mask"], st, RC.K_MAX, eps).any(), c["name"]
        near, exact = REF.near_ties(x, c["mask"], st, RC.K_MAX), REF.exact_ties(x, c["mask"], st, RC.K_MAX)
        assert not (near & ~exact).any(), c["name"]                     # whatever near_ties flags is an exact tie
        if exact.any():
            assert c["family"] == "ties" or c.get("equal"), c["name"]
        if c["family"] == "ties":
            live = [i for i in c["tied"] if REF.allowed(c["mask"], c["state"], c["V"])[i]]
            assert exact[0, :len(live)].all() == (len(live) > 1) and not exact[0, len(live):].any(), c["name"]
    for g in RC.row_groups():
        for c in g["rows"]:
            assert not REF.unplanted_near_ties(c["logits"][None], g["shared"], [c["state"]], RC.K_MAX).any(), (g["name"], c["name"])
    assert [len(g["rows"]) for g in RC.row_groups()] == list(RC.ROW_COUNTS) * len(RC.ROW_SIZES)


def test_every_margin_pair_flips_the_winner():
    cases = [c for c in RC.single_cases() if c["family"] == "margin"]
    seen = set()
    for ts, text in zip(cases[0::2], cases[1::2]):
        assert ts["name"].rsplit("/", 1)[0] == text["name"].rsplit("/", 1)[0] and ts["sign"] > 0 > text["sign"]
        tb = ts["state"]["timestamp_begin"]
        for c in (ts, text):
            ok = REF.allowed(c["mask"], c["state"], c["V"])
            x = c["logits"].astype(np.float64)
            got = RC.lse64(x[tb:][ok[tb:]]) - x[:tb][ok[:tb]].max()
            assert got == pytest.approx(c["margin"], rel=1e-3, abs=4 * np.spacing(np.float32(80))), c["name"]
            others = np.flatnonzero(ok[:tb])
            others = others[others != c["plant"]]
            assert len(others) == 0 or x[others].max() <= x[c["plant"]] - 1.0, c["name"]
        assert winner(ts)[0] >= tb and winner(text)[0] == text["plant"] == ts["plant"], ts["name"]
        seen.add((abs(ts["margin"]), ts["V"]))
    assert len(seen) == len(RC.MARGINS) * len(RC.SIZES)


def test_every_border_case_has_the_forbidden_token_on_top_and_an_allowed_winner():
    cases = [c for c in RC.single_cases() if c["family"] == "borders"]
    labels = {c["name"].rsplit("/", 1)[1] for c in cases}
    assert {"mask0_up", "mask1_first", "mask1_later", "nt_set_down", "nt_none", "mode1", "mode2", "bound_tb", "bound_mid", "bound_v",
            "first_tb", "initial0", "initial50", "initial_none", "without"} <= labels
    forbidden_on_top = 0
    for c in cases:
        ok = REF.allowed(c["mask"], c["state"], c["V"])
        assert int(c["logits"].argmax()) == c["top"], c["name"]
        assert winner(c)[0] == c["winner"] and ok[c["winner"]], c["name"]
        if c["top"] != c["winner"]:
            assert not ok[c["top"]], c["name"]
            forbidden_on_top += 1
    assert forbidden_on_top >= len(cases) * 2 // 3


def test_tie_and_degenerate_cases_say_what_they_plant():
    for c in RC.single_cases():
        if c["family"] == "ties":
            assert len({c["logits"][i].tobytes() for i in c["tied"]}) == 1 and c["logits"].max() == c["logits"][c["tied"][0]]
            assert winner(c)[0] == c["winner"], c["name"]
        if c.get("single"):
            assert winner(c) == (c["winner"], 0.0), c["name"]
        if c.get("peak") is not None:
            assert c["logits"].max() == np.float32(c["peak"])
    three = [c for c in RC.single_cases() if c["name"].endswith("three_waves")]
    assert three and all(len({(i % 1024) // 64 for i in c["tied"]}) == 3 for c in three)
    few = [c for c in RC.single_cases() if "few_" in c["name"]]
    assert few and all(REF.allowed(c["mask"], c["state"], c["V"]).sum() < RC.K_MAX for c in few)
    assert any(REF.rules_topk_reference(c["logits"][None], c["mask"], [c["state"]], 8)[1][0, 1] == -1 for c in few)


def test_the_float32_restatement_follows_float64():
    worst = 0.0
    for c in RC.single_cases()[::7]:
        lp, ids = REF.rules_topk_reference(c["logits"][None], c["mask"], [c["state"]], 8)
        lp32 = REF.rules_topk_f32(c["logits"][None], c["mask"], [c["state"]], ids)
        assert np.array_equal(np.isfinite(lp32), np.isfinite(lp)), c["name"]
        fin = np.isfinite(lp)
        worst = max(worst, float(np.abs(lp32[fin] - lp[fin]).max()))
    assert worst < 2e-5, worst


# ---- history_state --------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def real_vocab(tmp_path, monkeypatch):
    monkeypatch.setenv("WLK_VOCAB_DIR", H.real_vocab_dir(tmp_path))
    monkeypatch.setenv("WLK_SYNTHETIC_VOCAB", "0")


def _of(dec, history):
    nt = -1 if dec.tok.no_timestamps is None else int(dec.tok.no_timestamps)
    mi = -1 if dec.max_initial_ts is None else int(dec.max_initial_ts)
    return REF.history_state(history, dec.tok.timestamp_begin, dec.tok.eot, nt, mi, bool(dec.o.without_timestamps))


def test_history_state_is_the_hosts_pick_state(real_vocab):
    model = WG.PickingOracleModel(WG.MODEL, WG.SEED)
    cases = WB.transition_cases(model)
    assert len(cases) > 2000
    for dec, h, t in cases:
        for hist in (h, h + [t]):
            want = {f: int(v) for f, v in WB.state_of(dec, hist).items()}
            assert _of(dec, hist) == want, (hist, want)


def test_the_host_transition_walks_every_short_history():
    """transcribe._next_pick_state (the host statement of common.h's pick_rules_advance) over every history the GPU test
    walks on the device"""
    levels = RC.walk_levels()
    assert [len(l) for l in levels] == [len(RC.WALK_ALPHABET) ** n for n in range(RC.WALK_LEN + 1)] and len(RC.WALK_ALPHABET) == 6
    for mi in (0, -1):
        for wt in (0, 1):
            for level in levels[1:]:
                for h in level:
                    got = TR._next_pick_state(RC.walk_state(h[:-1], mi, wt), h[-1])
                    assert {f: int(v) for f, v in got.items()} == RC.walk_state(h, mi, wt), (h, mi, wt)


def test_the_draft_histories_obey_the_rules_and_take_every_transition():
    for V in RC.DRAFT_SIZES:
        mask, seen = RC.base_mask(V), set()
        for i in range(3):
            h = RC.draft_history(V, i)
            assert len(h) == RC.DRAFT_LEN and RC.layout(V)["eot"] not in h
            states = [RC.state_after(V, h[:j]) for j in range(len(h) + 1)]
            for j, t in enumerate(h):
                assert REF.allowed(mask, states[j], V)[t], (V, i, j)
                assert not any(REF.allowed(mask, states[j], V)[d] for d in RC.decoys(states[j], V)), (V, i, j)
            seen |= {(a["first_step"], a["ts_mode"], b["ts_mode"]) for a, b in zip(states, states[1:])}
            for m in RC.DRAFT_MISMATCH:
                if m is not None:
                    o = RC.other_token(V, h, m)
                    assert o != h[m] and REF.allowed(mask, states[m], V)[o]
                    assert m == 0 or RC.state_after(V, h[:m] + [o]) == states[m + 1]
        assert seen == {(1, 0, 1), (0, 1, 0), (0, 0, 2), (0, 2, 1), (0, 0, 0), (0, 2, 0)}, seen


# ---- the diagnostic entries refuse before they upload ---------------------------------------------------------------------------
def test_the_diag_entries_refuse_bad_arguments():
    lib = _lib.load()
    V = 16
    x = np.zeros((2, V), np.float32)
    mask = np.zeros(V, np.uint8)
    good = np.asarray([[0, 0, 10, 8, 9, 0, 10, 50]] * 2, np.int32)
    tok, bits = np.zeros(1, np.int32), np.zeros(1, np.uint32)
    lp, ids = np.zeros((2, 8), np.float32), np.zeros((2, 8), np.int32)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def one(**kw):
        a = dict(x=x, V=V, mask=mask, p=good, tok=tok, bits=bits)
        a.update(kw)
        return lib.wlk_diag_pick_one(vp(a["x"]), a["V"], vp(a["mask"]), vp(a["p"]), vp(a["tok"]), vp(a["bits"]))

    def topk(**kw):
        a = dict(x=x, V=V, mask=mask, p=good, n=2, k=2, lp=lp, ids=ids)
        a.update(kw)
        return lib.wlk_diag_pick_topk(vp(a["x"]), a["V"], vp(a["mask"]), vp(a["p"]), a["n"], a["k"], vp(a["lp"]), vp(a["ids"]))

    def bad(**fields):
        p = good.copy()
        for f, v in fields.items():
            p[-1, RC.FIELDS.index(f)] = v
        return p
    params = [bad(timestamp_begin=-1), bad(timestamp_begin=V + 1), bad(eot=-1), bad(eot=V), bad(ts_mode=3), bad(ts_mode=-1)]
    for key in ("x", "mask", "p", "tok", "bits"):
        assert one(**{key: None}) == WLK_ERR_ARG, key
    for key in ("x", "mask", "p", "lp", "ids"):
        assert topk(**{key: None}) == WLK_ERR_ARG, key
    assert one(V=0) == WLK_ERR_ARG and topk(V=0) == WLK_ERR_ARG
    for kw in (dict(n=0), dict(n=9), dict(k=0), dict(k=9), dict(n=-1), dict(k=-1)):
        assert topk(**kw) == WLK_ERR_ARG, kw
    for p in params:
        assert one(p=p[-1:].copy()) == WLK_ERR_ARG and topk(p=p) == WLK_ERR_ARG, p[-1]
    assert tok[0] == 0 and bits[0] == 0 and not lp.any() and not ids.any()
