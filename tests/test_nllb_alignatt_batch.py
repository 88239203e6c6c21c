"""AlignAtt through the stacked batch on the CPU: the batch stand-in against `transformers`' own
cross-attention (tests/golden/nllb_align_kat.npz), `nllb.generate_alignatt_batch` against the 78 stored outcomes and
over a scripted batch, the serving front (`NllbAlignAttStacker`, `HipAlignAttTranslation` over a stacked model), and the
refusals that need no device.  The gpu-marked twins (tests/test_gpu_nllb_alignatt_batch.py) run the library."""
import ctypes as C
import os
import re
import threading

import numpy as np
import pytest

import helpers as H
import nllb_align_standin as A
import nllb_alignatt_batch_standin as B
from nllb_align_standin import align_gain_state_dict
from oracle.nllb_oracle import NllbOracle
from whisperlivekit_amd import _lib, nllb
from whisperlivekit_amd import translation as T
from whisperlivekit_amd.policy import ASRToken

KAT = H.golden_npz("nllb_align_kat.npz")
N_CASES = int(KAT["n_cases"])
CFG = nllb.NLLB_MICRO
EOS = CFG.eos_token_id
P_ATOL = 5e-5          # the bound tests/test_nllb_alignatt.py holds the session stand-in to
JOIN_S = 120
NEW_SYMBOLS = ("wlk_nllb_batch_set_align", "wlk_nllb_batch_prefill", "wlk_nllb_batch_step_align", "wlk_nllb_batch_align_stats",
               "wlk_diag_nllb_align_rows")


@pytest.fixture(scope="module")
def micro_oracle():
    return NllbOracle(CFG, align_gain_state_dict(CFG, 0))


# ---- 1. the stand-in against the fixture -----------------------------------------------------------------------------------
def test_standin_batch_matches_transformers_in_six_slots_at_once(micro_oracle):
    assert N_CASES == 6
    batch = B.AlignOracleNllbBatch(micro_oracle, 8)
    batch.set_alignment_heads(KAT["heads"].tolist())
    slots = [5, 0, 7, 2, 3, 6]                                  # case ci lives in slots[ci]
    srcs = [KAT[f"c{ci}_src"] for ci in range(N_CASES)]
    greedy = [KAT[f"c{ci}_greedy"].tolist() for ci in range(N_CASES)]
    n_steps = len(greedy[0])
    assert all(len(g) == n_steps for g in greedy)
    batch.encode(slots, srcs)
    batch.prefill(slots, [[CFG.decoder_start_token_id]] * N_CASES)
    toks = [int(KAT[f"c{ci}_lang"]) for ci in range(N_CASES)]
    for t in range(n_steps):
        _lp, ids, pos, prob, mass = batch.step_align(slots, toks, 1, [1] * N_CASES, [len(s) - 1 for s in srcs], [0] * N_CASES)
        for ci in range(N_CASES):
            want = KAT[f"c{ci}_p64"][t]
            p = batch.alignment(slots[ci])
            assert p.shape == (len(srcs[ci]),)
            np.testing.assert_allclose(p, want, rtol=0, atol=P_ATOL, err_msg=f"case {ci} step {t}")
            assert int(pos[ci]) == int(KAT[f"c{ci}_pos"][t]) and int(ids[ci, 0]) == greedy[ci][t], (ci, t)
            assert abs(float(prob[ci]) - want[int(pos[ci])]) <= P_ATOL and abs(float(mass[ci]) - want.sum()) <= P_ATOL
        toks = [g[t] for g in greedy]
    assert batch.n_align_steps == n_steps and batch.n_prefills == 1


# ---- 2. the stored outcomes through the batch loop ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_slots", [8, 3, 1])
@pytest.mark.parametrize("order", ["stored", "reversed"])
def test_generate_alignatt_batch_reproduces_the_stored_outcomes(micro_oracle, n_slots, order):
    reqs, want = B.all_requests(KAT, A.settings_of)
    assert len(reqs) == 78
    if order == "reversed":
        reqs, want = reqs[::-1], want[::-1]
    batch = B.AlignOracleNllbBatch(micro_oracle, n_slots)
    batch.set_alignment_heads(KAT["heads"].tolist())
    got = nllb.generate_alignatt_batch(batch, reqs)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"request {i} ({order}, {n_slots} slots): {reqs[i][2:]}"
    assert all(e is None for e in batch.enc)                     # every slot was released
    assert max(batch.align_rows) == min(n_slots, 78)
    if n_slots > 1:
        assert batch.n_steps < batch.n_rows                      # requests shared steps


# ---- 3. the rule over a scripted batch -----------------------------------------------------------------------------------------
def req(src, committed=(), n_acc=None, thr=0, final=False, max_new=199, bos=1991):
    return (list(src), bos, list(committed), len(src) if n_acc is None else n_acc, thr, final, max_new)


SRC7 = [1990, 10, 11, 12, 13, 14, EOS]


def scripted(n_slots=8, **kw):
    b = B.ScriptedAlignBatch(CFG, n_slots, **kw)
    b.set_alignment_heads([(0, 0)])
    return b


def test_every_stop_reason_in_one_pass_and_each_equals_the_session_rule():
    cases = [req(SRC7, n_acc=6, thr=2),                                   # attention after three tokens
             req(SRC7, n_acc=6, thr=0),                                   # eos, not final
             req(SRC7, n_acc=6, thr=0, final=True),                       # eos, final
             req(SRC7, n_acc=3, thr=9),                                   # stops at its FIRST step while the neighbours go on
             req(SRC7, n_acc=6, thr=0, max_new=2),                        # length
             req(SRC7, n_acc=6, thr=0, max_new=0),                        # no slot at all
             req(SRC7, committed=[1010, 1011], n_acc=2, thr=0, final=True),
             req(SRC7, committed=[1010, 1011], n_acc=6, thr=1),
             req([1990, EOS], n_acc=1),                                   # empty window: position -1
             req([1990, 10, 11, B.END_MARKER, 13, EOS], n_acc=3),         # </s> on a position past the limit: attention wins
             req([1990, 10, 11, B.END_MARKER, 13, EOS], n_acc=3, final=True)]
    want = [([1010, 1011, 1012], [1, 2, 3], "attention"), ([1010, 1011, 1012, 1013, 1014], [1, 2, 3, 4, 5], "eos"),
            ([1010, 1011, 1012, 1013, 1014], [1, 2, 3, 4, 5], "eos"), ([], [], "attention"), ([1010, 1011], [1, 2], "length"),
            ([], [], "length"), ([1012, 1013, 1014], [3, 4, 5], "eos"), ([1012, 1013], [3, 4], "attention"), ([], [], "attention"),
            ([1010, 1011], [1, 2], "attention"), ([1010, 1011], [1, 2], "eos")]
    batch = scripted(8)
    got = nllb.generate_alignatt_batch(batch, cases)
    assert got == want
    for c, w in zip(cases, want):                                         # ... which is generate_alignatt's answer, one by one
        src, bos, committed, n_acc, thr, final, max_new = c
        assert nllb.generate_alignatt(B.ScriptedAlignSession(CFG), src, bos, committed=committed, n_accessible=n_acc, threshold=thr,
                                      final=final, max_new_tokens=max_new, device_loop=False) == w
    # admission: the first eight workable requests share one encode and one prefill; max_new_tokens = 0 took no slot
    assert batch.encodes[0] == list(range(8)) and len(batch.prefills[0]) == 8
    assert batch.prefills[0][:5] == [1, 1, 1, 1, 1] and batch.prefills[0][5] == 3      # prompt[:-1]: </s> (+ language + committed - 1)
    assert batch.steps[0] == list(range(8))                               # final and non-final rows in one step
    assert batch.encodes[1] == [3, 7] and batch.prefills[1] == [1, 1]     # the two that stopped at once made room for the last two
    assert sorted(batch.released) == sorted(s for call in batch.encodes for s in call)
    assert all(s is None for s in batch.src)


def test_a_freed_slot_is_refilled_in_the_middle_of_a_pass():
    long_, short = req(SRC7, n_acc=6, thr=0, final=True), req(SRC7, n_acc=3, thr=9)
    batch = scripted(2)
    got = nllb.generate_alignatt_batch(batch, [long_, short, req(SRC7, committed=[1010], n_acc=6, thr=2), short])
    assert got == [([1010, 1011, 1012, 1013, 1014], [1, 2, 3, 4, 5], "eos"), ([], [], "attention"),
                   ([1011, 1012], [2, 3], "attention"), ([], [], "attention")]
    assert batch.encodes == [[0, 1], [1], [1]]                            # slot 1 was freed and taken twice while slot 0 ran on
    assert batch.prefills == [[1, 1], [2], [1]]                           # the joiner's prompt [</s>, language, 1010]: two rows
    assert batch.steps[0] == [0, 1] and batch.steps[1] == [0, 1] and [0] in batch.steps


def test_a_prompt_of_exactly_two_tokens_prefills_one_row():
    batch = scripted(1)
    assert nllb.generate_alignatt_batch(batch, [req(SRC7, n_acc=6, thr=2)]) == [([1010, 1011, 1012], [1, 2, 3], "attention")]
    assert batch.prefills == [[1]] and len(batch.steps) == 4


def test_more_and_done_join_a_running_pass():
    batch = scripted(2)
    later = [[(*req(SRC7, n_acc=6, thr=2), "t0")], [], [(*req(SRC7, n_acc=6, thr=0, max_new=0), "t1"), (*req(SRC7, n_acc=3, thr=9), "t2")]]
    polls, outcomes = [], {}

    def more():
        polls.append(len(batch.steps))
        return later.pop(0) if later else None

    got = nllb.generate_alignatt_batch(batch, [req(SRC7, n_acc=6, thr=0)], more=more, done=lambda t, o: outcomes.__setitem__(t, o))
    assert got == [([1010, 1011, 1012, 1013, 1014], [1, 2, 3, 4, 5], "eos")]
    assert outcomes == {"t0": ([1010, 1011, 1012], [1, 2, 3], "attention"), "t1": ([], [], "length"), "t2": ([], [], "attention")}
    assert polls[:3] == [0, 1, 2] and batch.steps[0] == [0, 1]            # polled once per step; t0 joined the first step
    assert nllb.generate_alignatt_batch(batch, [], more=lambda: None) == []


def test_context_stop_and_bad_requests():
    batch = scripted(2, max_tgt=5)
    got = nllb.generate_alignatt_batch(batch, [req(SRC7, n_acc=6, thr=0, final=True), req(SRC7, committed=[1010, 1011, 1012], final=True),
                                               req(SRC7, committed=[1010, 1011, 1012, 1013], final=True)])
    assert got == [([1010, 1011, 1012, 1013], [1, 2, 3, 4], "context"), ([1013], [4], "context"), ([], [], "context")]
    assert batch.prefills == [[1, 4]]                                     # a prompt longer than the context takes no slot
    sess = B.ScriptedAlignSession(CFG)
    sess.model.cdims = batch.model.cdims
    assert nllb.generate_alignatt(sess, SRC7, 1991, n_accessible=6, threshold=0, final=True, device_loop=False) == got[0]
    for bad in (req(SRC7, n_acc=8), req(SRC7, thr=-1), req(SRC7, max_new=-1)):
        with pytest.raises(ValueError):
            nllb.generate_alignatt_batch(scripted(2), [bad])


def test_context_stop_over_the_standin(micro_oracle):
    batch = B.AlignOracleNllbBatch(micro_oracle, 2, max_tgt=64)
    batch.set_alignment_heads(KAT["heads"].tolist())
    src = KAT["c3_src"].tolist()
    (ids, al, why), = nllb.generate_alignatt_batch(batch, [req(src, final=True, bos=int(KAT["c3_lang"]))])
    assert why == "context" and len(ids) == 63 and len(al) == 63 and CFG.pad_token_id not in ids


# ---- 4. serving --------------------------------------------------------------------------------------------------------------
def words(spec, t0=0.0):
    return [ASRToken(start=round(t0 + 0.4 * i, 2), end=round(t0 + 0.4 * i + 0.4, 2), text=" " + w) for i, w in enumerate(spec.split())]


def stream_sentence(tm, target="fra_Latn"):
    """A.SENTENCE word by word with a two-word hypothesis tail, then a tail-only update, then the last word -> the
    (validated text, buffer text) of every call"""
    toks = words(A.SENTENCE)
    assert len(toks) == 12
    now = [0.0]
    tr = tm.new_session("eng_Latn", target)
    tr._clock = lambda: now[0]
    log = []
    for i, w in enumerate(toks[:-1]):
        now[0] += 1.0
        tr.insert_tokens([w, A.HypothesisTail(" ".join(t.text.strip() for t in toks[i + 1:i + 3]))])
        log.append(tr.process())
    now[0] += 1.0
    tr.insert_tokens([A.HypothesisTail(toks[-1].text.strip() + " and")])
    log.append(tr.process())
    tr.insert_tokens(toks[-1:])
    log.append(tr.process())
    log.append(tr.validate_buffer_and_reset())
    texts = [(None if new is None else (new.start, new.end, new.text), buf.text) for new, buf in log]
    counts = (tr.updates, tr.finals)
    has_session = tr.session is not None
    tr.close()
    return texts, counts, has_session


def make_tm(model, **kw):
    return T.HipNllbTranslationModel(model, B.HashTokenizer(EOS), policy="alignatt", threshold=2, hypothesis_tail=True,
                                     max_new_tokens=24, **kw)


def run_threads(work, n):
    errors = []

    def guarded(i):
        try:
            work(i)
        except BaseException as e:       # noqa: BLE001 - reported by the caller
            errors.append(e)

    threads = [threading.Thread(target=guarded, args=(i,), daemon=True) for i in range(n)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(JOIN_S)
    assert not any(th.is_alive() for th in threads), "a thread hangs"
    return errors


def test_eight_stacked_sessions_equal_their_unstacked_twin(monkeypatch):
    monkeypatch.delenv("WLK_NLLB_STACK", raising=False)
    plain_model = B.ScriptedAlignModel(CFG)
    want, want_counts, has_session = stream_sentence(make_tm(plain_model))
    assert has_session and plain_model.batches == [] and want[-2][0] is not None and any(buf for _new, buf in want[:-2])
    model = B.ScriptedAlignModel(CFG)
    tm = make_tm(model, stack=8)
    assert isinstance(tm.stacker, T.NllbAlignAttStacker) and model.batches[0].n_slots == 8
    assert model.batches[0].heads == nllb.default_alignment_heads(CFG)
    got = [None] * 8
    errors = run_threads(lambda i: got.__setitem__(i, stream_sentence(tm, ["fra_Latn", "deu_Latn"][i % 2])), 8)
    assert not errors, errors
    for i in range(8):
        texts, counts, has_session = got[i]
        assert texts == want and counts == want_counts and not has_session, i
    assert model.sessions == []                                           # no device session anywhere
    assert tm.stacker.sentences == 8 * sum(want_counts)
    assert 0 < tm.stacker.passes <= tm.stacker.sentences
    assert all(s is None for s in model.batches[0].src)
    tm.close()
    assert model.batches[0].closed and tm.stacker is None


def test_a_failing_pass_wakes_every_waiter_and_the_next_call_works():
    state = {"armed": True}
    box = {}

    def on_step(batch, slots):
        stacker = box["tm"].stacker
        if state["armed"] and len(batch.steps) >= 2:
            with stacker._cv:                                             # every caller has handed its request in
                ready = stacker._next_ticket >= 8
            if ready or len(batch.steps) >= 100000:
                state["armed"] = False
                raise RuntimeError("injected device failure")

    long_src = [1990] + list(range(10, 70)) + [EOS]

    class Endless(B.ScriptedAlignBatch):                                  # rows that never stop on their own while armed
        def step_align(self, slots, tokens, k, lo, hi, limit):
            lp, ids, pos, prob, mass = super().step_align(slots, tokens, k, lo, hi, limit)
            if state["armed"]:
                for s in slots:
                    self.fed[s] = self.fed[s][:2]                         # the copy starts over: same token again and again
            return lp, ids, pos, prob, mass

    model = B.ScriptedAlignModel(CFG, on_step=on_step)
    model.new_batch = lambda n_slots=8: model.batches.append(Endless(CFG, n_slots, 0, on_step)) or model.batches[-1]
    tm = box["tm"] = make_tm(model, stack=4)
    outcomes = [None] * 8

    def work(i):
        try:
            outcomes[i] = ("ok", tm.stacker.decode_many([req(long_src, final=True, max_new=10 ** 9)]))
        except RuntimeError as e:
            outcomes[i] = ("raised", str(e))

    assert not run_threads(work, 8)
    assert outcomes == [("raised", "injected device failure")] * 8, outcomes
    assert all(s is None for s in model.batches[0].src)                   # the failed pass left no slot occupied
    assert tm.stacker.decode_many([req(SRC7, n_acc=6, thr=2), req(SRC7, n_acc=6, thr=0)]) == [
        ([1010, 1011, 1012], [1, 2, 3], "attention"), ([1010, 1011, 1012, 1013, 1014], [1, 2, 3, 4, 5], "eos")]
    assert tm.stacker.decode_many([]) == []


def test_stack_unset_keeps_the_session_and_local_agreement_keeps_its_stacker(micro_oracle, monkeypatch):
    monkeypatch.delenv("WLK_NLLB_STACK", raising=False)
    for kw in ({}, {"stack": 0}):
        model = B.ScriptedAlignModel(CFG)
        tm = make_tm(model, **kw)
        tr = tm.new_session("eng_Latn", "fra_Latn")
        assert tm.stack == 0 and tm.batch is None and tm.stacker is None and model.batches == []
        assert isinstance(tr, T.HipAlignAttTranslation) and tr.session is model.sessions[0]
        assert tr.session.heads == nllb.default_alignment_heads(CFG)
    monkeypatch.setenv("WLK_NLLB_STACK", "3")                               # the environment stacks this policy too
    model = B.ScriptedAlignModel(CFG)
    tm = make_tm(model, alignment_heads=[(0, 1)])
    assert tm.stack == 3 and isinstance(tm.stacker, T.NllbAlignAttStacker) and model.batches[0].heads == [(0, 1)]
    assert tm.new_session("eng_Latn", "fra_Latn").session is None and model.sessions == []
    monkeypatch.delenv("WLK_NLLB_STACK")
    # policy="local_agreement", stack=n: NllbStacker over a batch without heads, as before
    import types
    from nllb_batch_standin import OracleNllbBatch
    batches = []
    greedy_model = types.SimpleNamespace(cfg=CFG, new_batch=lambda n: batches.append(OracleNllbBatch(micro_oracle, n)) or batches[-1])
    tm = T.HipNllbTranslationModel(greedy_model, B.HashTokenizer(EOS), stack=2)
    assert type(tm.stacker) is T.NllbStacker and batches[0].n_slots == 2 and not hasattr(batches[0], "heads")
    assert type(tm.new_session("eng_Latn", "fra_Latn")) is T.HipOnlineTranslation


# ---- 5. refusals without a device ------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_documented():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    declared = set(re.findall(r"\b(wlk_[a-z_0-9]+)\s*\(", open(os.path.join(root, "include", "wlk_hip.h")).read()))
    integration = open(os.path.join(root, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), name), name
        assert name in integration, name


def test_refusals_need_no_device():
    """WLK_ERR_ARG (-1), not WLK_ERR_HIP, on a machine without a GPU - and nothing is written"""
    import nllb_align_cases as AC
    lib = _lib.load()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)           # noqa: E731
    probs = AC.random_probs(2, 2, 16, 0)
    out = np.full(64, np.nan, np.float32)
    pos = np.full(8, -7, np.int32)
    i32 = lambda *v: np.asarray(v, np.int32)               # noqa: E731
    ok = dict(n=2, rows=2, stride=16, S=i32(9, 16), lo=i32(1, 0), hi=i32(8, 16), limit=i32(0, 16))
    for change in (dict(n=0), dict(n=65), dict(rows=0), dict(rows=9), dict(stride=0), dict(stride=513), dict(S=i32(0, 16)),
                   dict(S=i32(9, 17)), dict(lo=i32(1, -1)), dict(hi=i32(10, 16)), dict(hi=i32(8, 17)), dict(limit=i32(-1, 0)),
                   dict(limit=i32(0, 17)), dict(limit=i32(10, 0))):
        a = dict(ok, **change)
        rc = lib.wlk_diag_nllb_align_rows(ptr(probs), a["n"], a["rows"], a["stride"], ptr(a["S"]), ptr(a["lo"]), ptr(a["hi"]),
                                          ptr(a["limit"]), ptr(out), ptr(pos), ptr(out), ptr(out))
        assert rc == -1, change
    a = ok
    assert lib.wlk_diag_nllb_align_rows(None, 2, 2, 16, ptr(a["S"]), ptr(a["lo"]), ptr(a["hi"]), ptr(a["limit"]), ptr(out), ptr(pos),
                                        ptr(out), ptr(out)) == -1
    assert lib.wlk_diag_nllb_align_rows(ptr(probs), 2, 2, 16, None, ptr(a["lo"]), ptr(a["hi"]), ptr(a["limit"]), ptr(out), ptr(pos),
                                        ptr(out), ptr(out)) == -1
    assert np.isnan(out).all() and (pos == -7).all()
    # the batch entry points: a NULL batch or argument is refused before anything touches a device
    pairs, u64 = i32(0, 0), C.c_uint64()
    assert lib.wlk_nllb_batch_set_align(None, ptr(pairs), 1) == -1 and b"NULL" in lib.wlk_last_error()
    assert lib.wlk_nllb_batch_prefill(None, ptr(pos), ptr(pos), ptr(pos), 1) == -1
    assert lib.wlk_nllb_batch_step_align(None, ptr(pos), ptr(pos), 1, 1, ptr(pos), ptr(pos), ptr(pos), ptr(out), ptr(pos), ptr(pos),
                                         ptr(out), ptr(out)) == -1
    assert lib.wlk_nllb_batch_align_stats(None, C.byref(u64), C.byref(u64)) == -1
    assert np.isnan(out).all() and (pos == -7).all()
