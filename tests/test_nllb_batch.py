"""NLLB: several different sentences per launch chain - `HipNllbBatch` / `generate_batch` / the opt-in stacking of
translation.py - against `transformers`' single-sentence answers (tests/golden/nllb_batch_kat.npz,
scripts/gen_golden_nllb_batch.py).  What is pinned: a sentence translated in a stacked pass gives exactly what it gives
alone, whichever other sentences share its launches, in whichever slot, admitted at whichever step.

CPU part: the host loop and the serving glue over an oracle-backed stand-in for the batch (nllb_batch_standin.py).
GPU part: the library (csrc/nllb_batch.hip)."""
import ctypes as C
import threading
import types

import numpy as np
import pytest
import torch

import helpers as H
from nllb_batch_standin import OracleNllbBatch
from oracle.nllb_oracle import NllbOracle, OracleNllbSession
from test_translation import LANGS, WordTokenizer, words
from whisperlivekit_amd import _lib, nllb
from whisperlivekit_amd import translation as T

KAT = H.golden_npz("nllb_batch_kat.npz")
CFG = nllb.NLLB_MICRO
CASES = [tuple(int(v) for v in row) for row in KAT["cases"]]           # (source length, language id, max_new_tokens)
N = len(CASES)
SRC = [KAT[f"src{i}"] for i in range(N)]
GEN = [KAT[f"gen{i}"].tolist() for i in range(N)]
LANG = [c[1] for c in CASES]
LIMIT = [c[2] for c in CASES]
WEIGHTS = dict(seed=int(KAT["seed"]), eos_gain=float(KAT["eos_gain"]))
ENC_ATOL, LOGIT_ATOL = 2e-4, 1e-3      # tests/test_nllb.py's tolerances of the one-sentence path
ROW_ATOL = 2e-5                        # test_hip_rows_and_reorder's rows-versus-one-row figure
JOIN_S = 120                           # no thread of these tests may take longer; one that does is reported, not waited for


def _weights():
    return nllb.synth_state_dict(CFG, WEIGHTS["seed"], WEIGHTS["eos_gain"])


@pytest.fixture(scope="module")
def oracle():
    return NllbOracle(CFG, _weights())


def test_fixture_covers_what_the_tests_need():
    """A drifted fixture must not hollow the tests out: the length mix, own languages / limits, early and late endings."""
    assert N >= 12
    lens = [len(s) for s in SRC]
    assert lens == [c[0] for c in CASES]
    assert 1 in lens and 90 in lens and sum(1 for n in lens if 1 < n < 10) >= 3 and any(64 <= n < 90 for n in lens)
    assert len(lens) - len(set(lens)) >= 1                                  # two of equal length
    assert len(set(LANG)) >= 8 and len(set(LIMIT)) >= 8 and all(4 <= m <= 40 for m in LIMIT)
    early = [i for i in range(N) if GEN[i][-1] == CFG.eos_token_id and len(GEN[i]) < 1 + LIMIT[i]]
    at_limit = [i for i in range(N) if len(GEN[i]) == 1 + LIMIT[i] and GEN[i][-1] != CFG.eos_token_id]
    assert len(early) >= 3 and len(at_limit) >= 3, (early, at_limit)
    for i in range(N):
        assert KAT[f"logits{i}"].shape == (4, CFG.vocab_size) and KAT[f"enc{i}"].shape == (lens[i], CFG.d_model)
        assert GEN[i][:2] == [CFG.decoder_start_token_id, LANG[i]]


ORDERS = [list(range(N)), [9, 3, 0, 11, 8, 1, 10, 5, 2, 7, 4, 6]]


@pytest.mark.parametrize("n_slots", [8, 3, 1])
@pytest.mark.parametrize("order", range(len(ORDERS)))
def test_generate_batch_over_the_stand_in_equals_single_sentences(oracle, n_slots, order):
    """8 slots (4 sentences wait), 3 slots (refill in the middle of a decode), 1 slot (no stacking at all), two orders."""
    idx = ORDERS[order]
    batch = OracleNllbBatch(oracle, n_slots)
    got = nllb.generate_batch(batch, [SRC[i] for i in idx], [LANG[i] for i in idx], max_new_tokens=[LIMIT[i] for i in idx])
    assert got == [GEN[i] for i in idx]
    assert all(e is None for e in batch.enc), "every slot is released at the end of a pass"
    assert batch.n_rows == sum(len(GEN[i]) - 1 for i in idx)               # one row per generated token, none wasted
    if n_slots > 1:
        assert batch.n_steps < batch.n_rows
    else:
        assert batch.n_steps == batch.n_rows and batch.n_encodes == N


def test_generate_batch_options_match_generate(oracle):
    """Scalar arguments, forced </s> at each sentence's own limit, no forced language, a zero limit, and work handed in
    through `more`."""
    sess = OracleNllbSession(oracle, 1)
    batch = OracleNllbBatch(oracle, 4)
    idx = [2, 4, 6, 9, 0]
    want = [nllb.generate(sess, SRC[i], LANG[i], max_new_tokens=LIMIT[i], forced_eos_token_id=CFG.eos_token_id) for i in idx]
    assert nllb.generate_batch(batch, [SRC[i] for i in idx], [LANG[i] for i in idx], max_new_tokens=[LIMIT[i] for i in idx],
                               forced_eos_token_id=CFG.eos_token_id) == want
    want = [nllb.generate(sess, SRC[i], None, max_new_tokens=7) for i in idx]
    assert nllb.generate_batch(batch, [SRC[i] for i in idx], None, max_new_tokens=7) == want
    assert nllb.generate_batch(batch, [SRC[1], SRC[2]], 1990, max_new_tokens=[0, 3]) == [
        [CFG.decoder_start_token_id], nllb.generate(sess, SRC[2], 1990, max_new_tokens=3)]
    with pytest.raises(ValueError):
        nllb.generate_batch(batch, [SRC[1], SRC[2]], [1990], max_new_tokens=3)
    late, polls, base = {}, [], batch.n_steps

    def more():
        polls.append(batch.n_steps - base)
        if len(polls) == 3:                                 # joins a running pass at its third step
            return [(SRC[5], LANG[5], LIMIT[5], "a"), (SRC[8], LANG[8], LIMIT[8], "b")]
        return None

    got = nllb.generate_batch(batch, [SRC[3], SRC[1]], [LANG[3], LANG[1]], max_new_tokens=[LIMIT[3], LIMIT[1]], more=more,
                              done=lambda ticket, ids: late.__setitem__(ticket, ids))
    assert got == [GEN[3], GEN[1]] and late == {"a": GEN[5], "b": GEN[8]}
    assert polls[:4] == [0, 1, 2, 3]                        # once per step


# ---- serving glue over a fake model --------------------------------------------------------------------------------
class OracleModel:
    """What HipNllbTranslationModel needs from a HipNllbModel (tests/test_translation.py's fake, plus new_batch)."""
    def __init__(self, oracle, on_step=None):
        self.cfg, self.oracle, self.on_step = CFG, oracle, on_step
        self.batches = []

    def new_session(self, rows=1):
        s = OracleNllbSession(self.oracle, rows)
        s.close = lambda: None
        return s

    def new_batch(self, n_slots=8):
        self.batches.append(OracleNllbBatch(self.oracle, n_slots, self.on_step))
        return self.batches[-1]


VOCAB = "the quick brown fox jumps over lazy dog and then it sleeps hello again friend new sentence here last words".split()


def session_script(i):
    """A word stream of its own per session: bursts of 1..4 words, sentence ends, a silence and a speaker change."""
    rng = np.random.default_rng(100 + i)
    script, t = [], 0.0
    for step in range(9):
        n = int(rng.integers(1, 5))
        burst = [VOCAB[int(k)] for k in rng.integers(0, len(VOCAB), size=n)]
        for j in range(n):
            if rng.random() < 0.25:
                burst[j] += "."
        script.append(("tokens", words(" ".join(burst), t)))
        t += 0.4 * n
        if step == 4:
            script.append(("silence_start", None))
        if step == 6:
            script.append(("speaker", None))
    script.append(("tokens", []))
    return script


def drive(tm, script, target):
    tr = tm.new_session("eng_Latn", target)
    log = []
    for kind, arg in script:
        if kind == "tokens":
            tr.insert_tokens(arg)
            new, buf = tr.process()
        else:
            new, buf = tr.validate_buffer_and_reset()
        assert isinstance(buf, T.TimedText) and (new is None or isinstance(new, T.Translation))
        log.append((kind, None if new is None else (new.start, new.end, new.text), (buf.start, buf.end, buf.text)))
    n = tr.translations
    tr.close()
    return log, n


def run_sessions(tm, n_sessions=8):
    """n sessions on n threads, as AudioProcessor runs them; -> per-session (log, translations)."""
    targets = ["fra_Latn", "deu_Latn"]
    out, errors = [None] * n_sessions, []

    def work(i):
        try:
            out[i] = drive(tm, session_script(i), targets[i % 2])
        except BaseException as e:       # noqa: BLE001 - reported by the caller
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(n_sessions)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(JOIN_S)
    assert not any(th.is_alive() for th in threads), "a session thread hangs"
    if errors:
        raise errors[0]
    return out


def test_stacked_sessions_equal_their_unstacked_twins(oracle, monkeypatch):
    monkeypatch.delenv("WLK_NLLB_STACK", raising=False)
    plain = T.HipNllbTranslationModel(OracleModel(oracle), WordTokenizer(), max_new_tokens=12, stack=0)
    want = [drive(plain, session_script(i), ["fra_Latn", "deu_Latn"][i % 2]) for i in range(8)]
    model = OracleModel(oracle)
    tm = T.HipNllbTranslationModel(model, WordTokenizer(), max_new_tokens=12, stack=8)
    assert tm.stacker is not None and model.batches[0].n_slots == 8
    got = run_sessions(tm)
    assert [g[0] for g in got] == [w[0] for w in want]                 # Translation and buffer sequences, session by session
    assert [g[1] for g in got] == [w[1] for w in want]                 # translations are still counted per segment
    n_translations = sum(g[1] for g in got)
    assert tm.stacker.sentences == n_translations
    assert 0 < tm.stacker.passes < n_translations, (tm.stacker.passes, n_translations)
    assert model.batches[0].n_steps < model.batches[0].n_rows          # sentences of different sessions shared steps
    tm.close()
    assert model.batches[0].closed and tm.stacker is None


def test_a_failing_pass_wakes_every_waiter(oracle):
    """A batch that raises in the middle of a pass: the runner and all queued callers raise, nobody hangs, and the next
    request runs on a fresh pass."""
    state = {"armed": True}
    tm_box = {}

    def on_step(batch, slots):
        stacker = tm_box["tm"].stacker
        if state["armed"] and batch.n_steps >= 2:
            with stacker._cv:                                          # every caller has handed its requests in
                ready = stacker._next_ticket >= 8
            if ready or batch.n_steps >= 200:
                state["armed"] = False
                raise RuntimeError("injected device failure")

    tm = tm_box["tm"] = T.HipNllbTranslationModel(OracleModel(oracle, on_step), WordTokenizer(), max_new_tokens=400, stack=4)
    outcomes = [None] * 8

    def work(i):
        try:
            outcomes[i] = ("ok", tm.stacker.translate_many([(SRC[3 + i % 4], LANG[i], 400)]))
        except RuntimeError as e:
            outcomes[i] = ("raised", str(e))

    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(JOIN_S)
    assert not any(th.is_alive() for th in threads), "a waiter blocks for ever"
    assert outcomes == [("raised", "injected device failure")] * 8, outcomes
    assert all(e is None for e in tm.model.batches[0].enc)             # the failed pass left no slot occupied
    assert tm.stacker.translate_many([(SRC[2], LANG[2], LIMIT[2]), (SRC[4], LANG[4], LIMIT[4])]) == [GEN[2], GEN[4]]
    assert tm.stacker.translate_many([]) == []


def test_stacking_is_off_by_default(oracle, monkeypatch):
    monkeypatch.delenv("WLK_NLLB_STACK", raising=False)
    for kw in ({}, {"stack": 0}, {"stack": 8, "num_beams": 3}):        # beams keep their own sessions
        model = OracleModel(oracle)
        tm = T.HipNllbTranslationModel(model, WordTokenizer(), **kw)
        assert tm.stack == 0 and tm.batch is None and tm.stacker is None and model.batches == []
        assert tm.new_session("eng_Latn", "fra_Latn").session is not None
        tm.close()
    monkeypatch.setenv("WLK_NLLB_STACK", "3")
    model = OracleModel(oracle)
    tm = T.HipNllbTranslationModel(model, WordTokenizer())
    assert tm.stack == 3 and model.batches[0].n_slots == 3 and tm.new_session("eng_Latn", "fra_Latn").session is None
    assert T.HipNllbTranslationModel(OracleModel(oracle), WordTokenizer(), stack=0).stacker is None     # the argument wins
    with pytest.raises(ValueError):
        T.HipNllbTranslationModel(OracleModel(oracle), WordTokenizer(), stack=9)


def test_abi_exports_the_batch_entry_points():
    lib = _lib.load()
    for name in ("wlk_nllb_batch_create", "wlk_nllb_batch_destroy", "wlk_nllb_batch_encode", "wlk_nllb_batch_step",
                 "wlk_nllb_batch_release", "wlk_nllb_batch_export", "wlk_nllb_batch_cross_attention", "wlk_nllb_batch_sync"):
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS
    out = C.c_void_p()
    assert lib.wlk_nllb_batch_create(None, 4, C.byref(out)) != 0 and not out.value
    assert b"NULL" in lib.wlk_last_error()
    for call in (lambda: lib.wlk_nllb_batch_sync(None), lambda: lib.wlk_nllb_batch_release(None, 0)):
        assert call() != 0 and lib.wlk_last_error()
    assert lib.wlk_nllb_batch_destroy(None) == 0


# ---- the HIP library --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def micro_hip():
    m = nllb.HipNllbModel.from_hf_state_dict(CFG, _weights(), device=0, max_src=92, max_tgt=64)
    yield m
    m.close()


@pytest.mark.gpu
def test_hip_create_needs_a_finalized_model():
    lib = _lib.load()
    m = nllb.HipNllbModel(CFG, device=0, max_src=92, max_tgt=64)           # created, nothing uploaded
    try:
        out = C.c_void_p()
        assert lib.wlk_nllb_batch_create(m._h, 4, C.byref(out)) != 0 and not out.value
        assert b"finalized" in lib.wlk_last_error()
        with pytest.raises(_lib.WlkError):
            m.new_batch(4)
    finally:
        m.close()


@pytest.mark.gpu
def test_hip_stacked_encoder_matches_transformers(micro_hip):
    """All sentences in stacked calls of 8 and 4; the second call takes four slots of the first and leaves the others alone."""
    batch = micro_hip.new_batch(8)
    try:
        batch.encode(list(range(8)), SRC[:8])
        for s in range(8):
            err = float(np.abs(batch.encoder_output(s) - KAT[f"enc{s}"]).max())
            print(f"stack of 8, sentence {s} ({len(SRC[s])} ids): encoder error {err:.3g}")
            np.testing.assert_allclose(batch.encoder_output(s), KAT[f"enc{s}"], rtol=0, atol=ENC_ATOL)
        taken = [6, 1, 4, 3]
        batch.encode(taken, SRC[8:12])
        for s, i in zip(taken, range(8, 12)):
            err = float(np.abs(batch.encoder_output(s) - KAT[f"enc{i}"]).max())
            print(f"stack of 4, sentence {i} ({len(SRC[i])} ids) in slot {s}: encoder error {err:.3g}")
            np.testing.assert_allclose(batch.encoder_output(s), KAT[f"enc{i}"], rtol=0, atol=ENC_ATOL)
        for s in (0, 2, 5, 7):
            np.testing.assert_allclose(batch.encoder_output(s), KAT[f"enc{s}"], rtol=0, atol=ENC_ATOL)
    finally:
        batch.close()


@pytest.mark.gpu
@pytest.mark.parametrize("group", [[2, 3, 5, 6, 7, 8, 9, 11], [10, 0, 4, 1]])
def test_hip_stacked_steps_match_transformers(micro_hip, group):
    """Teacher-forced first 4 steps of stacked sentences (5 .. 90 source ids side by side) against the per-sentence logits."""
    batch = micro_hip.new_batch(8)
    try:
        slots = list(range(len(group)))
        batch.encode(slots, [SRC[i] for i in group])
        for step in range(4):
            lp, ids = batch.step(slots, [int(KAT[f"fed{i}"][step]) for i in group], 4)
            for s, i in zip(slots, group):
                want = KAT[f"logits{i}"][step]
                got = batch.logits(s)
                print(f"step {step}, sentence {i}: logit error {float(np.abs(got - want).max()):.3g}")
                np.testing.assert_allclose(got, want, rtol=0, atol=LOGIT_ATOL, err_msg=f"sentence {i} step {step}")
                ref = torch.log_softmax(torch.from_numpy(want), dim=-1)
                np.testing.assert_allclose(lp[s], ref.topk(4)[0].numpy(), rtol=0, atol=LOGIT_ATOL)
                assert ids[s, 0] == int(ref.argmax()) or abs(float(ref[ids[s, 0]] - ref.max())) < H.TIE_EPS
    finally:
        batch.close()


@pytest.mark.gpu
def test_hip_rows_do_not_depend_on_their_neighbours(micro_hip):
    """Row r of a stack of 8 against the same sentence alone in a 1-slot batch and in a HipNllbSession."""
    group = [9, 0, 3, 8, 5, 4, 7, 2]
    many, one, sess = micro_hip.new_batch(8), micro_hip.new_batch(1), micro_hip.new_session(1)
    try:
        many.encode(list(range(8)), [SRC[i] for i in group])
        stacked = [many.step(list(range(8)), [int(KAT[f"fed{i}"][step]) for i in group], 4) for step in range(4)]
        for r, i in enumerate(group):
            one.encode([0], [SRC[i]])
            sess.encode(SRC[i])
            for step in range(4):
                tok = int(KAT[f"fed{i}"][step])
                lp1, ids1 = one.step([0], [tok], 4)
                sess.decode(np.asarray([[tok]], np.int64), first=(step == 0))
                lps, idss = sess.topk(4)
                lp8, ids8 = stacked[step][0][r], stacked[step][1][r]
                print(f"sentence {i} step {step}: |stack - alone| {float(np.abs(lp8 - lp1[0]).max()):.3g}, "
                      f"|stack - session| {float(np.abs(lp8 - lps[0]).max()):.3g}")
                np.testing.assert_allclose(lp8, lp1[0], rtol=0, atol=ROW_ATOL)
                np.testing.assert_allclose(lp8, lps[0], rtol=0, atol=ROW_ATOL)
                assert ids8.tolist() == ids1[0].tolist() == idss[0].tolist()
            one.release(0)
    finally:
        many.close(); one.close(); sess.close()


@pytest.mark.gpu
def test_hip_ragged_cross_attention_is_bitwise_row_independent(micro_hip):
    """The ragged cross-attention kernel alone: a row's output bits are the same alone, in a stack of 8, in another order
    and in a subset - and they are the softmax-weighted values of that row's own keys (checked through a one-hot query)."""
    group = [0, 1, 4, 5, 6, 8, 9, 11]                                  # 1, 3, 9, 9, 17, 64, 90, 20 keys
    batch = micro_hip.new_batch(8)
    try:
        batch.encode(list(range(8)), [SRC[i] for i in group])
        rng = np.random.default_rng(5)
        q = rng.standard_normal((8, CFG.d_model)).astype(np.float32)
        for layer in range(CFG.decoder_layers):
            full = batch.cross_attention(list(range(8)), layer, q)
            assert np.isfinite(full).all()
            for s in range(8):
                alone = batch.cross_attention([s], layer, q[s:s + 1])
                assert alone.tobytes() == full[s:s + 1].tobytes(), (layer, s)
            order = [5, 2, 7, 0, 6, 3]
            mixed = batch.cross_attention(order, layer, q[order])
            assert mixed.tobytes() == full[order].tobytes()
            # a sentence of ONE key returns that key's value row whatever the query (softmax over one score = 1): slot 0 gives
            # the same bits for another query - a kernel that read a neighbour's key count would mix in rows that are not there
            a = batch.cross_attention([0], layer, q[3:4])
            assert a.tobytes() == full[0:1].tobytes()
    finally:
        batch.close()


def _hip_generate_all(model, n_slots, idx):
    batch = model.new_batch(n_slots)
    try:
        return nllb.generate_batch(batch, [SRC[i] for i in idx], [LANG[i] for i in idx], max_new_tokens=[LIMIT[i] for i in idx])
    finally:
        batch.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_slots", [8, 3])
def test_hip_generate_batch_matches_transformers(micro_hip, n_slots):
    for idx in ORDERS:
        assert _hip_generate_all(micro_hip, n_slots, idx) == [GEN[i] for i in idx]


@pytest.mark.gpu
def test_hip_generate_batch_with_a_tight_target_context():
    """max_tgt = the longest output + 1: the last step of the longest sentence lands on the cache's last rows."""
    longest = max(len(g) for g in GEN)
    model = nllb.HipNllbModel.from_hf_state_dict(CFG, _weights(), device=0, max_src=92, max_tgt=longest + 1)
    try:
        assert _hip_generate_all(model, 8, ORDERS[1]) == [GEN[i] for i in ORDERS[1]]
    finally:
        model.close()


@pytest.mark.gpu
def test_hip_batch_reused_for_other_lengths(micro_hip):
    """One batch object, three rounds with different length mixes: nothing of a recorded step graph may remember a source
    length or a position (the session's graph did: wlk_nllb_session::step_exec_src).  Each round == fresh 1-row generate."""
    batch = micro_hip.new_batch(4)
    try:
        for idx in ([2, 6, 0, 9], [9, 8, 7, 1], [4, 5, 10, 3, 11, 0]):
            want = []
            for i in idx:
                fresh = micro_hip.new_session(1)
                try:
                    want.append(nllb.generate(fresh, SRC[i], LANG[i], max_new_tokens=LIMIT[i]))
                finally:
                    fresh.close()
            got = nllb.generate_batch(batch, [SRC[i] for i in idx], [LANG[i] for i in idx], max_new_tokens=[LIMIT[i] for i in idx])
            assert got == want, idx
            assert want == [GEN[i] for i in idx]
    finally:
        batch.close()


@pytest.mark.gpu
def test_hip_batch_rejects_bad_input_and_stays_usable():
    model = nllb.HipNllbModel.from_hf_state_dict(CFG, _weights(), device=0, max_src=92, max_tgt=6)
    batch = model.new_batch(3)
    E = _lib.WlkError
    try:
        with pytest.raises(E):
            model.new_batch(0)
        with pytest.raises(E):
            model.new_batch(9)
        with pytest.raises(E):
            batch.step([0], [2])                                      # not encoded
        with pytest.raises(E):
            batch.encode([0, 0], [SRC[1], SRC[2]])                    # a slot twice
        with pytest.raises(E):
            batch.encode([0, 3], [SRC[1], SRC[2]])                    # slot out of range
        with pytest.raises(E):
            batch.encode([0], [[5, 1, 6]])                            # padding inside a sentence
        with pytest.raises(E):
            batch.encode([0], [[5] * 93])                             # longer than max_src
        with pytest.raises(E):
            batch.encode([0], [[]])                                   # empty sentence
        with pytest.raises(E):
            batch.encode([0], [[5, 99999, 2]])                        # token out of range
        with pytest.raises(E):
            batch.encode([0, 1, 2, 0], [SRC[1]] * 4)                  # more sentences than slots
        batch.encode([0, 2], [SRC[1], SRC[4]])
        with pytest.raises(E):
            batch.step([0, 0], [2, 2])                                # a slot twice
        with pytest.raises(E):
            batch.step([0, 1], [2, 2])                                # slot 1 is not encoded
        with pytest.raises(E):
            batch.step([0], [99999])
        with pytest.raises(E):
            batch.step([0], [CFG.pad_token_id])
        with pytest.raises(E):
            batch.step([], [])                                        # R outside 1..8
        with pytest.raises(E):
            batch.step([0, 2], [2, 2], 9)                             # k above the top-k kernel's limit
        with pytest.raises(E):
            batch.logits(0)                                           # no step yet
        with pytest.raises(E):
            batch.release(5)
        # after all that the batch still translates: slots 0 and 2 as encoded above, against the fixture's logits
        for step in range(4):
            batch.step([2, 0], [int(KAT["fed4"][step]), int(KAT["fed1"][step])], 1)
            np.testing.assert_allclose(batch.logits(2), KAT["logits4"][step], rtol=0, atol=LOGIT_ATOL)
            np.testing.assert_allclose(batch.logits(0), KAT["logits1"][step], rtol=0, atol=LOGIT_ATOL)
        batch.step([2], [7], 1)
        batch.step([2], [8], 1)                                       # position 5 = max_tgt - 1
        with pytest.raises(E):
            batch.step([2], [9], 1)                                   # max_tgt exceeded
        with pytest.raises(E):
            batch.logits(0)                                           # slot 0 was not in the latest step
        batch.release(2)
        with pytest.raises(E):
            batch.step([2], [2], 1)                                   # released
        batch.encode([2], [SRC[1]])
        batch.step([2], [int(KAT["fed1"][0])], 1)
        np.testing.assert_allclose(batch.logits(2), KAT["logits1"][0], rtol=0, atol=LOGIT_ATOL)
    finally:
        batch.close()
        model.close()


@pytest.mark.gpu
def test_hip_stacked_serving_equals_unstacked(micro_hip, monkeypatch):
    """8 HipOnlineTranslation sessions on 8 threads over one 8-slot batch: the same validated pieces and buffers as each
    session alone on its own 1-row device session."""
    monkeypatch.delenv("WLK_NLLB_STACK", raising=False)
    plain = T.HipNllbTranslationModel(micro_hip, WordTokenizer(), max_new_tokens=12, stack=0)
    want = [drive(plain, session_script(i), ["fra_Latn", "deu_Latn"][i % 2]) for i in range(8)]
    tm = T.HipNllbTranslationModel(micro_hip, WordTokenizer(), max_new_tokens=12, stack=8)
    try:
        got = run_sessions(tm)
        assert [g[0] for g in got] == [w[0] for w in want]
        assert [g[1] for g in got] == [w[1] for w in want]
        assert 0 < tm.stacker.passes < sum(g[1] for g in got)
    finally:
        tm.close()


@pytest.mark.gpu
def test_hip_600m_shape_stacked_steps_match_the_session():
    """NLLB-200-distilled-600M's dimensions, seeded weights: 8 sources of mixed length, 6 stacked greedy steps; every row
    against a 1-row HipNllbSession fed the same tokens (5e-3: test_hip_600m_shape_matches_the_oracle's tolerance)."""
    cfg = nllb.NLLB_200_DISTILLED_600M
    model = nllb.HipNllbModel.from_hf_state_dict(cfg, nllb.synth_state_dict(cfg, 1), device=0, max_src=64, max_tgt=32)
    batch, sess = model.new_batch(8), model.new_session(1)
    try:
        rng = np.random.default_rng(3)
        lens = [3, 64, 9, 22, 40, 5, 57, 14]
        srcs = [np.concatenate([[256047], rng.integers(4, 250000, size=n - 2), [2]]).astype(np.int64) for n in lens]
        batch.encode(list(range(8)), srcs)
        fed = [[2] * 8, [256057 + r for r in range(8)]]               # start token, then a target language per row
        got = []
        for step in range(6):
            lp, ids = batch.step(list(range(8)), fed[step], 2)
            got.append((lp, ids))
            if step >= 1:
                fed.append([int(t) for t in ids[:, 0]])                # greedy from here on
        for r in range(8):
            sess.encode(srcs[r])
            for step in range(6):
                sess.decode(np.asarray([[fed[step][r]]], np.int64), first=(step == 0))
                lps, idss = sess.topk(2)
                lp8, ids8 = got[step][0][r], got[step][1][r]
                print(f"row {r} ({lens[r]} ids) step {step}: |stack - session| {float(np.abs(lp8 - lps[0]).max()):.3g}")
                np.testing.assert_allclose(lp8, lps[0], rtol=0, atol=5e-3)
                assert int(ids8[0]) == int(idss[0, 0]) or abs(float(lps[0, 0] - lps[0, 1])) < H.TIE_EPS
    finally:
        batch.close(); sess.close(); model.close()
