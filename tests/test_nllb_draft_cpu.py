"""NLLB draft verification, the host side: `nllb.generate_batch(drafts=...)`, `nllb.clamp_draft`, the
serving glue of translation.py and the fixture tests/golden/nllb_draft_kat.npz - over a stand-in batch whose `verify` is one
teacher-forced decode of the CPU oracle (nllb_draft_cases.VerifyingOracleNllbBatch).

What is pinned: a draft changes how many tokens a pass yields, never which - every result equals `generate_batch` without
drafts, whatever the draft holds - and the rows stepped afterwards are exactly the tokens behind the accepted prefix."""
import os
import threading

import numpy as np
import pytest

import nllb_draft_cases as DC
from nllb_batch_standin import OracleNllbBatch
from oracle.nllb_oracle import NllbOracle, OracleNllbSession
from test_translation import WordTokenizer, words
from whisperlivekit_amd import _lib, nllb
from whisperlivekit_amd import translation as T

FX = DC.Fixture()
CFG = DC.CFG
EOS, START = CFG.eos_token_id, CFG.decoder_start_token_id
NEW_SYMBOLS = ("wlk_nllb_batch_verify", "wlk_nllb_batch_verify_stats", "wlk_diag_nllb_verify_pick")


@pytest.fixture(scope="module")
def oracle():
    return NllbOracle(CFG, FX.micro_weights())


def test_fixture_keeps_the_gap_and_covers_what_the_tests_need():
    """The stored gaps are the float64 oracle's, every truth is its own greedy continuation and keeps gap >= 2e-3; the mix of
    endings and lengths the tests rely on is there."""
    o64 = DC.float64_oracle(CFG, FX.micro_weights())
    assert float(FX.z["gap_min"]) == DC.GAP_MIN == 2e-3
    for i in range(FX.n):
        picks, gaps = DC.forced_gaps(o64, FX.src[i], FX.gen[i])
        assert picks == FX.gen[i][2:], i
        assert FX.gen[i][:2] == [START, FX.lang[i]] and len(FX.gap[i]) == len(FX.gen[i]) - 2
        np.testing.assert_allclose(gaps, FX.gap[i], rtol=0, atol=1e-9)
        assert float(gaps.min()) >= DC.GAP_MIN, (i, float(gaps.min()))
        assert len(FX.gen[i]) <= DC.MAX_TGT - 1 and (FX.gen[i][-1] == EOS or len(FX.gen[i]) == 1 + FX.limit[i])
        assert EOS not in FX.gen[i][1:-1]
    eos_ended = [i for i in range(FX.n) if FX.ends_by_eos(i) and len(FX.gen[i]) >= 12]
    at_limit = [i for i in range(FX.n) if len(FX.gen[i]) == 1 + FX.limit[i] and FX.gen[i][-1] != EOS]
    assert len(eos_ended) >= 2 and len(at_limit) >= 3, (eos_ended, at_limit)
    assert len(FX.gen[FX.long_case()]) >= 70 and FX.long_case() in at_limit
    assert 11 <= len(FX.big["gen"]) <= 14 and len(FX.big["gap"]) == len(FX.big["gen"]) - 2


def test_fixture_600m_truth_keeps_its_gap():
    """The 600M-shape truth recomputed by the float64 oracle in one teacher-forced pass: gap >= 1e-2."""
    import torch
    torch.set_num_threads(8)
    b = FX.big
    assert float(FX.z["big_gap_min"]) == DC.BIG_GAP_MIN == 1e-2
    o64 = DC.float64_oracle(DC.BIG_CFG, nllb.synth_state_dict(DC.BIG_CFG, b["seed"]))
    picks, gaps = DC.forced_gaps(o64, b["src"], b["gen"])
    assert picks == b["gen"][2:] and b["gen"][:2] == [2, b["lang"]]
    np.testing.assert_allclose(gaps, b["gap"], rtol=0, atol=1e-9)
    assert float(gaps.min()) >= DC.BIG_GAP_MIN
    assert len(b["gen"]) <= DC.BIG_MAX_TGT - 1 and len(b["src"]) <= DC.BIG_MAX_SRC


# ---- generate_batch(drafts=...) ------------------------------------------------------------------------------------------
def plain(oracle, idx, n_slots=8, **kw):
    batch = OracleNllbBatch(oracle, n_slots)
    return nllb.generate_batch(batch, [FX.src[i] for i in idx], [FX.lang[i] for i in idx], max_new_tokens=[FX.limit[i] for i in idx], **kw)


def drafted(oracle, idx, drafts, n_slots=8, **kw):
    batch = DC.VerifyingOracleNllbBatch(oracle, n_slots)
    got = nllb.generate_batch(batch, [FX.src[i] for i in idx], [FX.lang[i] for i in idx], max_new_tokens=[FX.limit[i] for i in idx],
                              drafts=drafts, **kw)
    assert all(e is None for e in batch.enc), "every slot is released at the end of a pass"
    return got, batch


def with_wrong(ids, at):
    out = list(ids)
    out[2 + at] = 7 if out[2 + at] != 7 else 8
    return out


def test_plain_generate_batch_gives_the_fixture(oracle):
    assert plain(oracle, list(range(FX.n))) == FX.gen


def test_exact_previous_result_is_accepted_whole(oracle):
    idx = list(range(FX.n))
    got, batch = drafted(oracle, idx, [FX.gen[i] for i in idx])
    assert got == FX.gen
    for call in batch.verify_calls:
        for _slot, k, n_d in call:
            assert k == n_d
    # rows stepped = the tokens behind the accepted prefix: the verify yields 2 + k + 1 ids, every later id is one stepped row
    want_rows = 0
    for i in idx:
        d = nllb.clamp_draft(FX.gen[i], FX.limit[i], DC.MAX_TGT, EOS)
        want_rows += len(FX.gen[i]) - (3 + len(d)) if d else len(FX.gen[i]) - 1
    assert batch.n_rows == want_rows and batch.n_accepted == batch.n_draft > 0


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_a_wrong_token_cuts_the_draft_there(oracle, where):
    idx = [i for i in range(FX.n) if len(FX.gen[i]) >= 8]
    drafts, at = [], {}
    for i in idx:
        n_d = len(nllb.clamp_draft(FX.gen[i], FX.limit[i], DC.MAX_TGT, EOS))
        at[i] = {"first": 0, "middle": n_d // 2, "last": n_d - 1}[where]
        drafts.append(with_wrong(FX.gen[i], at[i]))
    got, batch = drafted(oracle, idx, drafts)
    assert got == [FX.gen[i] for i in idx]
    accepted = {}
    for call in batch.verify_calls:
        for slot, k, _n_d in call:
            accepted.setdefault(slot, []).append(k)
    assert sorted(k for ks in accepted.values() for k in ks) == sorted(at.values())
    assert batch.n_rows == sum(len(FX.gen[i]) - (3 + at[i]) for i in idx)      # tokens behind the accepted prefix, none wasted


def test_drafts_that_run_past_the_end_garbage_and_empty_ones(oracle):
    eos_cases = [i for i in range(FX.n) if FX.ends_by_eos(i)]
    rng = np.random.default_rng(5)
    for i in eos_cases[:3]:
        past = FX.gen[i][:-1] + [11, 12, 13, 14]                        # no </s> where the truth has one: the pick there is </s>
        garbage = [START, FX.lang[i]] + rng.integers(4, 1900, size=20).tolist()
        invalid = FX.gen[i][:4] + [CFG.vocab_size + 5, -3, CFG.pad_token_id]     # cut where the library would refuse
        for draft in (past, garbage, invalid, [START, FX.lang[i]], [START], [], FX.gen[i][:3]):
            got, batch = drafted(oracle, [i], [draft])
            assert got == [FX.gen[i]], (i, draft)
        got, batch = drafted(oracle, [i], [past])
        assert batch.verify_calls == [[(0, len(FX.gen[i]) - 3, min(len(past) - 2, FX.limit[i] - 3))]]
        assert batch.n_rows == 0                                        # the verify's next token was </s>: no step at all
        got, batch = drafted(oracle, [i], [[START, FX.lang[i]]])
        assert batch.n_verifies == 0


def test_no_verify_at_tiny_limits_and_without_a_forced_language(oracle):
    sess = OracleNllbSession(oracle, 1)
    i = FX.long_case()
    for max_new in (0, 1, 2, 3):
        batch = DC.VerifyingOracleNllbBatch(oracle, 2)
        want = nllb.generate(sess, FX.src[i], FX.lang[i], max_new_tokens=max_new)
        assert nllb.generate_batch(batch, [FX.src[i]], FX.lang[i], max_new_tokens=max_new, drafts=[FX.gen[i]]) == [want]
        assert batch.n_verifies == 0
    batch = DC.VerifyingOracleNllbBatch(oracle, 2)
    want = nllb.generate(sess, FX.src[i], FX.lang[i], max_new_tokens=4)
    assert nllb.generate_batch(batch, [FX.src[i]], FX.lang[i], max_new_tokens=4, drafts=[FX.gen[i]]) == [want]
    assert batch.verify_calls == [[(0, 1, 1)]]
    batch = DC.VerifyingOracleNllbBatch(oracle, 2)                      # no forced BOS: the draft's second token is not forced
    want = nllb.generate(sess, FX.src[i], None, max_new_tokens=9)
    assert nllb.generate_batch(batch, [FX.src[i]], None, max_new_tokens=9, drafts=[want]) == [want]
    assert batch.n_verifies == 0
    with pytest.raises(ValueError):
        nllb.generate_batch(batch, [FX.src[i]], FX.lang[i], drafts=[None, None])


def test_forced_eos_at_each_sentences_own_limit(oracle):
    sess = OracleNllbSession(oracle, 1)
    idx = list(range(FX.n))
    want = [nllb.generate(sess, FX.src[i], FX.lang[i], max_new_tokens=FX.limit[i], forced_eos_token_id=EOS) for i in idx]
    for drafts in ([FX.gen[i] for i in idx], want, [with_wrong(FX.gen[i], 1) for i in idx]):
        got, batch = drafted(oracle, idx, drafts, forced_eos_token_id=EOS)
        assert got == want
        assert batch.n_verifies >= 1


def test_a_standin_without_verify_ignores_drafts(oracle):
    batch = OracleNllbBatch(oracle, 4)
    idx = [0, 3, 5]
    got = nllb.generate_batch(batch, [FX.src[i] for i in idx], [FX.lang[i] for i in idx], max_new_tokens=[FX.limit[i] for i in idx],
                              drafts=[FX.gen[i] for i in idx])
    assert got == [FX.gen[i] for i in idx] and batch.n_rows == sum(len(FX.gen[i]) - 1 for i in idx)


def test_drafts_and_none_mixed_over_three_slots_with_refills(oracle):
    idx = list(range(FX.n))
    drafts = [None if i % 3 == 0 else (FX.gen[i] if i % 3 == 1 else with_wrong(FX.gen[i], 2)) for i in idx]
    got, batch = drafted(oracle, idx, drafts, n_slots=3)
    assert got == FX.gen
    assert batch.n_encodes > 1 and batch.n_verifies > 1                 # refills in the middle of a decode verified too
    for call in batch.verify_calls:
        assert len(call) <= 3
    n_with = sum(1 for d in drafts if d is not None)
    assert sum(len(c) for c in batch.verify_calls) == n_with
    one_encode_one_verify = DC.VerifyingOracleNllbBatch(oracle, 8)
    nllb.generate_batch(one_encode_one_verify, [FX.src[i] for i in idx[:8]], [FX.lang[i] for i in idx[:8]],
                        max_new_tokens=[FX.limit[i] for i in idx[:8]], drafts=[FX.gen[i] for i in idx[:8]])
    assert one_encode_one_verify.n_encodes == 1 and one_encode_one_verify.n_verifies == 1


def test_five_tuples_through_more(oracle):
    batch = DC.VerifyingOracleNllbBatch(oracle, 4)
    late, polls = {}, []

    def more():
        polls.append(batch.n_steps)
        if len(polls) == 2:
            return [(FX.src[5], FX.lang[5], FX.limit[5], "a", FX.gen[5]), (FX.src[8], FX.lang[8], FX.limit[8], "b"),
                    (FX.src[9], FX.lang[9], FX.limit[9], "c", None), (FX.src[10], FX.lang[10], FX.limit[10], "d", with_wrong(FX.gen[10], 3))]
        return None

    got = nllb.generate_batch(batch, [FX.src[3], FX.src[1]], [FX.lang[3], FX.lang[1]], max_new_tokens=[FX.limit[3], FX.limit[1]],
                              more=more, done=lambda ticket, ids: late.__setitem__(ticket, ids), drafts=[FX.gen[3], None])
    assert got == [FX.gen[3], FX.gen[1]]
    assert late == {"a": FX.gen[5], "b": FX.gen[8], "c": FX.gen[9], "d": FX.gen[10]}
    assert sum(len(c) for c in batch.verify_calls) == 3


def test_clamp_draft_at_its_edges():
    prev = [2, 1990, 10, 11, 12, 13, 14, 2]
    assert nllb.clamp_draft(prev, 199, 80, 2) == [10, 11, 12, 13, 14]   # cut in front of </s>
    assert nllb.clamp_draft(prev[:-1], 199, 80, 2) == [10, 11, 12, 13, 14]
    assert nllb.clamp_draft(prev, 6, 80, 2) == [10, 11, 12]             # max_new_tokens - 3
    assert nllb.clamp_draft(prev, 4, 80, 2) == [10]
    assert nllb.clamp_draft(prev, 3, 80, 2) == [] and nllb.clamp_draft(prev, 0, 80, 2) == []
    assert nllb.clamp_draft(prev, 199, 5, 2) == [10, 11]                # max_tgt - 3: 2 + n_d <= max_tgt - 1
    assert nllb.clamp_draft(prev, 199, 3, 2) == []
    assert nllb.clamp_draft(prev, 199, None, 2) == [10, 11, 12, 13, 14]
    assert nllb.clamp_draft([2, 1990, 2], 199, 80, 2) == [] and nllb.clamp_draft([2, 1990], 199, 80, 2) == []
    assert nllb.clamp_draft([2], 199, 80, 2) == [] and nllb.clamp_draft([], 199, 80, 2) == [] and nllb.clamp_draft(None, 199, 80, 2) == []
    assert nllb.clamp_draft([2, 1990, 10, 2, 11, 2], 199, 80, 2) == [10]
    assert nllb.clamp_draft(np.asarray(prev), 199, 80, 2) == [10, 11, 12, 13, 14]
    # with that limit the token behind a fully accepted draft is never where the forced-</s> rule or the length stop decides
    for max_new in range(4, 12):
        n_d = len(nllb.clamp_draft([2, 1990] + [10] * 50, max_new, 80, 2))
        assert 2 + n_d <= (1 + max_new) - 2


# ---- serving glue ----------------------------------------------------------------------------------------------------------
class OracleModel:
    """What HipNllbTranslationModel needs from a HipNllbModel; its batches verify."""
    def __init__(self, oracle, verifying=True):
        self.cfg, self.oracle, self.verifying = CFG, oracle, verifying
        self.batches = []

    def new_session(self, rows=1):
        s = OracleNllbSession(self.oracle, rows)
        s.close = lambda: None
        return s

    def new_batch(self, n_slots=8):
        self.batches.append(DC.VerifyingOracleNllbBatch(self.oracle, n_slots) if self.verifying else OracleNllbBatch(self.oracle, n_slots))
        return self.batches[-1]


def test_draft_needs_a_stack_greedy_decoding_and_local_agreement(oracle, monkeypatch):
    monkeypatch.delenv("WLK_NLLB_DRAFT", raising=False)
    monkeypatch.delenv("WLK_NLLB_STACK", raising=False)
    for kw in (dict(stack=0), dict(stack=4, num_beams=2), dict(stack=4, policy="alignatt"), dict()):
        with pytest.raises(ValueError):
            T.HipNllbTranslationModel(OracleModel(oracle), WordTokenizer(), draft=True, **kw)
    model = OracleModel(oracle)
    tm = T.HipNllbTranslationModel(model, WordTokenizer(), stack=4)
    assert tm.draft is False                                            # off by default
    monkeypatch.setenv("WLK_NLLB_DRAFT", "1")
    assert T.HipNllbTranslationModel(OracleModel(oracle), WordTokenizer(), stack=4).draft is True
    assert T.HipNllbTranslationModel(OracleModel(oracle), WordTokenizer(), stack=4, draft=False).draft is False     # the argument wins
    with pytest.raises(ValueError):
        T.HipNllbTranslationModel(OracleModel(oracle), WordTokenizer())                 # the environment asks, nothing stacks
    monkeypatch.setenv("WLK_NLLB_DRAFT", "0")
    assert T.HipNllbTranslationModel(OracleModel(oracle), WordTokenizer(), stack=4).draft is False


def test_online_translation_with_drafts_gives_the_same_texts(oracle, monkeypatch):
    """A sentence growing word by word, a reset in the middle and a closing full stop (a screened script: every pick keeps the
    gap, see below): draft on == draft off, text by text; the previous hypothesis is the draft of the next update and of
    the final translation; accepted tokens > 0."""
    monkeypatch.delenv("WLK_NLLB_DRAFT", raising=False)
    script = DC.growing_script(**DC.RESET_SCRIPT)
    assert [kind for kind, _ in script].count("reset") == 1
    off = T.HipNllbTranslationModel(OracleModel(oracle), WordTokenizer(), max_new_tokens=DC.SCREENED_LIMIT, stack=2, draft=False)
    want, tr_off = DC.drive_script(off, script)
    assert tr_off._previous_ids is None and off.model.batches[0].n_verifies == 0        # no memory, no call with the switch off
    model = OracleModel(oracle)
    on = T.HipNllbTranslationModel(model, WordTokenizer(), max_new_tokens=DC.SCREENED_LIMIT, stack=2, draft=True)
    got, tr = DC.drive_script(on, script)
    assert got == want
    assert tr.translations == tr_off.translations                      # counted as before
    batch = model.batches[0]
    assert batch.n_verifies > 0 and batch.n_accepted > 0, (batch.n_verifies, batch.n_accepted)
    assert batch.n_rows < off.model.batches[0].n_rows                   # accepted tokens were not stepped
    print(f"growing sentence: {batch.n_verifies} verifies, {batch.n_accepted} of {batch.n_draft} draft tokens accepted, "
          f"{batch.n_rows} rows stepped against {off.model.batches[0].n_rows}")


def test_screened_growing_sentences_keep_the_gap_and_accept_tokens(oracle):
    """The sentences the GPU serving test compares text by text: every pick of every hypothesis keeps gap >= 2e-3 on the
    float64 oracle (so no kernel within tolerance turns a text), and their drafts are accepted in part."""
    o64 = DC.float64_oracle(CFG, FX.micro_weights())

    class Model:
        cfg = CFG

        def __init__(self, make):
            self.make, self.batches = make, []

        def new_batch(self, n_slots=8):
            self.batches.append(self.make(n_slots))
            return self.batches[-1]

    assert len(DC.SCREENED_SEEDS) >= 4
    runs = [(dict(seed=seed), target) for seed in DC.SCREENED_SEEDS for target in DC.SCREENED_TARGETS] + [(DC.RESET_SCRIPT, "fra_Latn")]
    for kw, target in runs:
        seed = kw["seed"]
        rec = Model(lambda n: DC.GapRecordingBatch(o64, n))
        tm = T.HipNllbTranslationModel(rec, WordTokenizer(), max_new_tokens=DC.SCREENED_LIMIT, stack=2)
        want, _ = DC.drive_script(tm, DC.growing_script(**kw), target)
        gaps = rec.batches[0].gaps
        assert len(gaps) >= 8 * 2 and min(gaps) >= DC.GAP_MIN, (seed, target, min(gaps))
        ver = Model(lambda n: DC.VerifyingOracleNllbBatch(oracle, n))
        tm = T.HipNllbTranslationModel(ver, WordTokenizer(), max_new_tokens=DC.SCREENED_LIMIT, stack=2, draft=True)
        got, _ = DC.drive_script(tm, DC.growing_script(**kw), target)
        assert got == want, (seed, target)
        assert ver.batches[0].n_accepted > 0, (seed, target)


def test_validate_buffer_and_reset_drops_the_memory(oracle):
    model = OracleModel(oracle)
    tm = T.HipNllbTranslationModel(model, WordTokenizer(), max_new_tokens=24, stack=2, draft=True)
    tr = tm.new_session("eng_Latn", "fra_Latn")
    tr.insert_tokens(words("the quick brown fox"))
    tr.process()
    assert tr._previous_ids is not None and tr._previous_ids[:2] == [START, 1991]
    before = model.batches[0].n_verifies
    tr.insert_tokens(words("jumps", 2.0))
    tr.process()
    assert model.batches[0].n_verifies == before + 1                    # the update carried the draft
    tr.validate_buffer_and_reset()
    assert tr._previous_ids is None and tr._previous == []
    tr.insert_tokens(words("hello again", 5.0))
    tr.process()
    assert model.batches[0].n_verifies == before + 1                    # a fresh segment has no draft
    tr.insert_tokens(words("friend.", 6.0))                             # punctuation closes it: the final translation takes the draft
    tr.process()
    assert model.batches[0].n_verifies == before + 2
    assert tr._previous_ids is None                                     # ... and the memory goes with the sentence


def test_stacker_requests_may_carry_a_draft(oracle):
    model = OracleModel(oracle)
    tm = T.HipNllbTranslationModel(model, WordTokenizer(), max_new_tokens=40, stack=4, draft=True)
    reqs = [(FX.src[1], FX.lang[1], FX.limit[1]), (FX.src[2], FX.lang[2], FX.limit[2], FX.gen[2]),
            (FX.src[4], FX.lang[4], FX.limit[4], None), (FX.src[5], FX.lang[5], FX.limit[5], with_wrong(FX.gen[5], 1))]
    assert tm.stacker.translate_many(reqs) == [FX.gen[1], FX.gen[2], FX.gen[4], FX.gen[5]]
    assert sum(len(c) for c in model.batches[0].verify_calls) == 2
    # a batch object without verify (the existing stand-ins) ignores drafts
    old = OracleModel(oracle, verifying=False)
    tm_old = T.HipNllbTranslationModel(old, WordTokenizer(), max_new_tokens=40, stack=4, draft=True)
    assert tm_old.stacker.translate_many(reqs) == [FX.gen[1], FX.gen[2], FX.gen[4], FX.gen[5]]


def test_four_threads_with_drafts_equal_their_draft_off_twins(oracle):
    runs = [(DC.SCREENED_SEEDS[i], DC.SCREENED_TARGETS[i % 2]) for i in range(4)]
    off = T.HipNllbTranslationModel(OracleModel(oracle), WordTokenizer(), max_new_tokens=DC.SCREENED_LIMIT, stack=4, draft=False)
    want = [DC.drive_script(off, DC.growing_script(seed), target)[0] for seed, target in runs]
    model = OracleModel(oracle)
    on = T.HipNllbTranslationModel(model, WordTokenizer(), max_new_tokens=DC.SCREENED_LIMIT, stack=4, draft=True)
    got, errors = [None] * 4, []

    def work(i):
        try:
            got[i] = DC.drive_script(on, DC.growing_script(runs[i][0]), runs[i][1])[0]
        except BaseException as e:       # noqa: BLE001 - reported below
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(120)
    assert not any(th.is_alive() for th in threads), "a session thread hangs"
    assert not errors, errors
    assert got == want
    assert model.batches[0].n_verifies > 0


def test_abi_exports_the_verify_entry_points():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wlk_hip.h")) as fh:
        header = fh.read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and f"int {name}(" in header, name
    assert lib.wlk_abi_version() == 2
    import ctypes as C
    u = C.c_uint64()
    assert lib.wlk_nllb_batch_verify(None, None, None, None, 1, None, None) == -1 and b"NULL" in lib.wlk_last_error()
    assert lib.wlk_nllb_batch_verify_stats(None, C.byref(u), C.byref(u), C.byref(u)) == -1
    assert lib.wlk_diag_nllb_verify_pick(None, 1, 7, None, None, None) == -1
