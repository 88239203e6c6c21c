"""NLLB beam search over device beam steps, the parts that need no GPU: `nllb.beam_search(device_steps=True)`
over a stand-in session that answers `step_beam` from the CPU oracle (tests/nllb_beam_standin.py) against `transformers`'
sequences, what the path calls and what it hands over, the switch, and the wide top-k kernel's selection scheme restated in
numpy against the float64 reference."""
import numpy as np
import pytest

import nllb_beam_standin as S
import select_reference as SR
from oracle.nllb_oracle import NllbOracle
from whisperlivekit_amd import nllb

CASES = S.beam_cases()
CASE_IDS = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def oracles():
    mk = lambda w: NllbOracle(nllb.NLLB_MICRO, nllb.synth_state_dict(nllb.NLLB_MICRO, w["seed"], w["eos_gain"]))
    return {"old": mk(S.OLD_WEIGHTS), "wide": mk(S.WIDE_WEIGHTS)}


def test_the_wide_golden_covers_what_it_is_for():
    rows = [c for c in CASES if c[1] == "wide"]
    assert sorted({c[4]["num_beams"] for c in rows}) == [5, 6, 7, 8]
    assert all(len(c[5]) - 1 >= 12 for c in rows)
    assert any(len(c[5]) - 1 < c[4]["max_new_tokens"] for c in rows)                 # a hypothesis that ended wins somewhere
    assert any(c[4]["length_penalty"] != 1.0 for c in rows) and any(c[4]["early_stopping"] is True for c in rows)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_device_steps_return_transformers_sequence(oracles, case):
    _, weights, src, lang, kw, want = case
    n = kw["num_beams"]
    dev = S.StandinNllbSession(oracles[weights], n)
    assert nllb.beam_search(dev, src, lang, device_steps=True, **kw) == want
    # the prompt is decode + topk(2 n); every later step one step_beam(…, 2 n); nothing else touches the device
    assert dev.calls("kv_reorder") == [] and dev.calls("logits") == [] and dev.calls("step") == []
    assert dev.calls("decode") == [("decode", True)] and dev.calls("topk") == [("topk", 2 * n)]
    steps = dev.calls("step_beam")
    assert all(e[2] == 2 * n for e in steps) and dev.beam_stats()["ancestry_steps"] == len(steps)
    # the sources handed over are, step by step, what the host path hands to kv_reorder (whose last call nothing reads)
    host = S.StandinNllbSession(oracles[weights], n)
    assert nllb.beam_search(host, src, lang, device_steps=False, **kw) == want
    assert host.calls("step_beam") == []
    reorders = [e[1] for e in host.calls("kv_reorder")]
    assert [e[1] for e in steps] == reorders[:-1]
    assert len(steps) >= 1


def test_the_switch_is_the_environment_and_off_by_default(oracles, monkeypatch):
    _, weights, src, lang, kw, want = CASES[0]
    monkeypatch.delenv("WLK_NLLB_BEAM_STEPS", raising=False)
    sess = S.StandinNllbSession(oracles[weights], kw["num_beams"])
    assert nllb.beam_search(sess, src, lang, **kw) == want
    assert sess.calls("step_beam") == [] and sess.calls("kv_reorder")
    monkeypatch.setenv("WLK_NLLB_BEAM_STEPS", "0")
    sess = S.StandinNllbSession(oracles[weights], kw["num_beams"])
    nllb.beam_search(sess, src, lang, **kw)
    assert sess.calls("step_beam") == []
    monkeypatch.setenv("WLK_NLLB_BEAM_STEPS", "1")
    sess = S.StandinNllbSession(oracles[weights], kw["num_beams"])
    assert nllb.beam_search(sess, src, lang, **kw) == want
    assert sess.calls("step_beam") and sess.calls("kv_reorder") == []
    # an explicit False beats the environment, and a session without step_beam takes the host path whatever is asked
    sess = S.StandinNllbSession(oracles[weights], kw["num_beams"])
    nllb.beam_search(sess, src, lang, device_steps=False, **kw)
    assert sess.calls("step_beam") == []
    from oracle.nllb_oracle import OracleNllbSession
    assert nllb.beam_search(OracleNllbSession(oracles[weights], kw["num_beams"]), src, lang, device_steps=True, **kw) == want


def test_standin_keeps_the_state_rule(oracles):
    sess = S.StandinNllbSession(oracles["old"], 3)
    sess.encode(S.KAT["beam_src0"])
    with pytest.raises(S.StateError):
        sess.step_beam([5, 6, 7], [0, 0, 0], 4)                   # before the prompt
    sess.decode(np.full((3, 1), 2, np.int64), first=True)
    sess.step([5, 6, 7], 2)
    sess.kv_reorder([1, 1, 0])
    sess.step_beam([8, 9, 10], [2, 0, 0], 16)
    for call in (lambda: sess.step([5, 6, 7], 2), lambda: sess.kv_reorder([0, 1, 2]),
                 lambda: sess.decode(np.full((3, 1), 9, np.int64), first=False)):
        with pytest.raises(S.StateError):
            call()
    assert sess.topk(16)[0].shape == (3, 16) and sess.logits().shape[0] == 3      # stay valid
    sess.decode(np.full((3, 1), 2, np.int64), first=True)
    sess.step([5, 6, 7], 2)
    sess.kv_reorder([0, 0, 1])


PLANTED = S.planted_rows()


@pytest.mark.parametrize("name", sorted(PLANTED))
def test_selection_scheme_against_float64(name):
    """64 slices, 256 strided owners of 16 entries, k exclusion rounds with owner rescan, 64-list merge: the ids are the
    float64 reference's (value descending, index ascending), -inf entries are never chosen."""
    x, k, n_finite = PLANTED[name]
    got = S.emulate_wide_topk(x, k)
    _, ids, gaps, _ = SR.logsoftmax_topk(x, None, k)
    n = k if n_finite is None else n_finite
    assert np.array_equal(got[:, :n], ids[:, :n]), (name, got, ids)
    assert (got[:, n:] == -1).all()
    if name == "ties":
        assert (gaps[:, :2] == 0).all()                           # the planted ties lead every row


@pytest.mark.parametrize("V,R,k,seed", [(4097, 3, 16, 0), (2003, 2, 10, 1), (1000, 2, 9, 2), (70001, 1, 16, 3)])
def test_selection_scheme_on_random_rows(V, R, k, seed):
    x = (np.random.default_rng(seed).standard_normal((R, V)) * 3).astype(np.float32)
    assert np.array_equal(S.emulate_wide_topk(x, k), SR.logsoftmax_topk(x, None, k)[1])


def test_selection_scheme_refuses_longer_rows():
    with pytest.raises(ValueError):
        S.emulate_wide_topk(np.zeros((1, 262145), np.float32), 4)


def test_filled_ranks_stay_in_their_row(oracles):
    """The wide kernel fills a row that has fewer than 2 n finite logits with (-inf, -1).  Such ranks must not alias another
    row's tokens in the flattened (beam, token) index: with the last ranks of every row replaced by the fill, the search
    still ranks real candidates only and returns the same sequence."""
    class Filled(S.StandinNllbSession):
        @staticmethod
        def _fill(out):
            lp, ids = (np.array(a) for a in out)
            keep = lp.shape[1] - 2
            lp[:, keep:], ids[:, keep:] = -np.inf, -1
            return lp, ids

        def topk(self, k):
            return self._fill(super().topk(k))

        def step_beam(self, tokens, sources, k):
            return self._fill(super().step_beam(tokens, sources, k))

    for case in CASES[:3]:
        _, weights, src, lang, kw, want = case
        sess = Filled(oracles[weights], kw["num_beams"])
        assert nllb.beam_search(sess, src, lang, device_steps=True, **kw) == want

    class Starved(Filled):
        """one finite candidate in all rows together: fewer than n, so the re-ranking has to pick fills"""
        @staticmethod
        def _fill(out):
            lp, ids = (np.array(a) for a in out)
            lp[:, 1:], ids[:, 1:] = -np.inf, -1
            lp[1:, 0], ids[1:, 0] = -np.inf, -1
            return lp, ids

    # a chosen fill is the padding token of its own row, which the next step refuses - not token V - 1 of the row before it
    _, weights, src, lang, kw, want = next(c for c in CASES if c[1] == "wide")
    assert want[2] != nllb.NLLB_MICRO.eos_token_id                 # the one real candidate of the first free step goes on
    with pytest.raises(ValueError, match="padding"):
        nllb.beam_search(Starved(oracles[weights], kw["num_beams"]), src, lang, device_steps=True, **kw)
