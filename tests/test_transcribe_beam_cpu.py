"""Batch `transcribe` with beam search on the device, the host half (no GPU): `_pick_states` + the float64 statement of
wlk_pick_topk's contract (tests/rules_topk_reference.py) against the host rules `_apply_rules` + top-k, and the device branch
of `_WindowDecoder.run` (WLK_TRANSCRIBE_DEVICE_BEAM=1) over an oracle-backed stand-in session against the host branch and
the reference's recorded beam result (tests/golden/transcribe_kat.json.gz: beam_then_best_of)."""
import numpy as np
import pytest

import helpers as H
from oracle_session import OracleModel, OracleSession
from rules_topk_reference import near_ties, rules_mask, rules_topk_reference
from whisperlivekit_amd import synth, transcribe as TR

KAT = H.golden_json("transcribe_kat.json")


@pytest.fixture()
def real_vocab(tmp_path, monkeypatch):
    monkeypatch.setenv("WLK_VOCAB_DIR", H.real_vocab_dir(tmp_path))
    monkeypatch.setenv("WLK_SYNTHETIC_VOCAB", "0")


def history_groups(tb, eot, rng):
    """Sampled-token histories by length; the rows of one group go through the rules in ONE call, so rows with different
    histories (no timestamp yet, an opening timestamp, a closed pair, text behind a pair ...) sit side by side."""
    text = lambda n: [int(t) for t in rng.integers(300, 20000, n)]
    return [
        [[], [], []],                                                        # first step: every row is the prompt
        [[tb], [tb + 3], text(1)],                                           # one timestamp (mode 1) beside one text token
        [[tb, *text(3)], [*text(4)], [tb, *text(2), tb + 40], [tb, *text(1), tb + 40, tb + 40],
         [tb, *text(2), tb + 1499], [tb, tb, *text(2)], [tb, *text(1), tb + 700, tb + 700][:4], [tb, *text(2), eot]],
        [[tb, *text(2), tb + 40, tb + 40, *text(1)], [tb, *text(3), tb + 900, tb + 900], [tb, *text(4), tb + 1500],
         [tb, *text(2), tb + 60, tb + 60, tb + 61], [*text(6)]],
    ]


def host_topk(dec, logits, tokens, k):
    """`_apply_rules` (fp32, the form followed against the reference's recorded choices) + the k best per row by
    (value descending, index ascending)."""
    lp = dec._apply_rules(logits.copy(), tokens)
    V = lp.shape[1]
    ids = np.stack([np.lexsort((np.arange(V), -row.astype(np.float64)))[:k] for row in lp])
    vals = np.take_along_axis(lp, ids, axis=1)
    return vals, np.where(np.isfinite(vals), ids, -1).astype(np.int32)


OPTIONS = [dict(), dict(without_timestamps=True), dict(suppress_blank=False, suppress_tokens=""),
           dict(max_initial_timestamp=None), dict(prompt="hello there", suppress_tokens="1,2,-1")]


@pytest.mark.parametrize("options", OPTIONS)
def test_pick_states_and_the_float64_contract_give_the_host_rules_topk(options, real_vocab):
    model = OracleModel("micro", 0)
    dec = TR._WindowDecoder(model, TR.DecodingOptions(language="en", temperature=0.0, beam_size=5, **options))
    V, tb, eot = model.dims.n_vocab, dec.tok.timestamp_begin, dec.tok.eot
    mask = rules_mask(V, dec.suppressed or [], dec.blank_ids or [])
    rng = np.random.default_rng(23)
    seen, n_cmp, n_tie = set(), 0, 0
    for group in history_groups(tb, eot, rng):
        tokens = np.asarray([list(dec.initial) + h for h in group], np.int64)
        for ts_lift in (0.0, 9.0):                    # text on top / the timestamps as a group on top
            logits = (rng.standard_normal((len(group), V)) * 3).astype(np.float32)
            logits[:, tb:] += np.float32(ts_lift)
            states = dec._pick_states(tokens)
            assert states[0] == dec._pick_state(tokens[:1]) == dec._pick_state(tokens)
            for k in (1, 6, 8):
                want_lp, want_id = host_topk(dec, logits, tokens, k)
                got_lp, got_id = rules_topk_reference(logits, mask, states, k)
                sure = ~near_ties(logits, mask, states, k)       # fp32 and float64 may rank a near-tie differently
                n_cmp += sure.size
                n_tie += int((~sure).sum())
                assert np.array_equal(got_id[sure], want_id[sure]), (options, group, k)
                fin = sure & (want_id >= 0)
                assert np.abs(got_lp[fin] - want_lp[fin]).max() <= 1e-5, (options, group, k)
                assert np.isneginf(got_lp[sure & (want_id < 0)]).all()
            for st, row in zip(states, want_id):
                seen.add((bool(st["first_step"]), st["ts_mode"], st["ts_bound"] > tb, bool((row[row >= 0] >= tb).all())))
    assert n_tie <= 0.02 * n_cmp, (n_tie, n_cmp)
    if not options.get("without_timestamps"):
        modes = {(f, m, b) for f, m, b, _ in seen}
        assert {(True, 0, False), (False, 0, False), (False, 0, True), (False, 1, True), (False, 2, True)} <= modes, modes
        assert {w for *_, w in seen} == {True, False}     # rows where the timestamps took over, and rows where they did not


def test_pick_states_of_rows_with_different_histories():
    """One call, a row in ts_mode 1 beside a row in ts_mode 2 with another bound: what the one-row block cannot express."""
    model = OracleModel("micro.en", 0)
    dec = TR._WindowDecoder(model, TR.DecodingOptions(language="en", temperature=0.0, beam_size=2))
    tb = dec.tok.timestamp_begin
    tokens = np.asarray([list(dec.initial) + [tb, 500, tb + 40, tb + 40], list(dec.initial) + [tb, 500, 600, tb + 77]], np.int64)
    a, b = dec._pick_states(tokens)
    assert (a["ts_mode"], a["ts_bound"]) == (1, tb + 41) and (b["ts_mode"], b["ts_bound"]) == (2, tb + 77)
    assert {k: v for k, v in a.items() if k not in ("ts_mode", "ts_bound")} == \
           {k: v for k, v in b.items() if k not in ("ts_mode", "ts_bound")}


# ---- the device branch of run() over a stand-in session ----------------------------------------------------------------
class BeamOracleSession(OracleSession):
    """OracleSession + the three calls of the device beam branch: `pick_topk` is the float64 contract over the oracle's
    logits (returned in fp32, as the device returns it), `decode_ancestry` is reorder + decode."""

    def __init__(self, model, beam):
        super().__init__(model, beam)
        self.mask = None
        self.calls = dict(set_rules=0, pick_topk=0, decode_ancestry=0, kv_reorder=0)

    def set_rules(self, suppressed, blank):
        self.calls["set_rules"] += 1
        self.mask = rules_mask(self.model.dims.n_vocab, suppressed, blank)

    def pick_topk(self, states, k):
        self.calls["pick_topk"] += 1
        assert len(states) == self.beam
        lp, ids = rules_topk_reference(self.logits_last.numpy(), self.mask, states, k)
        return lp.astype(np.float32), ids

    def decode_ancestry(self, last_tokens, sources):
        self.calls["decode_ancestry"] += 1
        self.cache.reorder(list(sources))
        self.decode(np.asarray(last_tokens, np.int64).reshape(-1, 1), first=False)

    def kv_reorder(self, source_rows):
        self.calls["kv_reorder"] += 1
        super().kv_reorder(source_rows)


def beam_case():
    case = next(c for c in KAT if c["name"] == "beam_then_best_of")
    assert case["model"] == "micro.en" and case["calls"][0]["beam"] == 3 and case["calls"][0]["temperature"] == 0
    kw = case["kwargs"]
    opts = dict(language=kw["language"], temperature=0.0, beam_size=kw["beam_size"], patience=kw["patience"],
                length_penalty=kw["length_penalty"])
    spec = case["audio"]
    audio = synth.white_noise(spec["seconds"], seed=spec["seed"])
    return case, opts, audio


def first_window(session, audio):
    """The first 30 s window as transcribe() cuts it: the content frames, filled up with zeros."""
    mel = session.log_mel(audio, padding=TR.N_SAMPLES)
    content = mel.shape[-1] - TR.N_FRAMES
    return TR.pad_or_trim(mel[:, :min(TR.N_FRAMES, content)])


def test_device_beam_branch_over_the_oracle_gives_the_host_branch_and_the_recorded_tokens(real_vocab, monkeypatch):
    case, opts, audio = beam_case()
    model = OracleModel(case["model"], 0)
    want = case["calls"][0]["result"]["tokens"]

    monkeypatch.delenv("WLK_TRANSCRIBE_DEVICE_BEAM", raising=False)
    host_s = BeamOracleSession(model, 3)
    host = TR.decode(model, first_window(host_s, audio), session=host_s, **opts)
    assert host_s.calls["pick_topk"] == 0 and host_s.calls["decode_ancestry"] == 0 and host_s.calls["kv_reorder"] > 0

    monkeypatch.setenv("WLK_TRANSCRIBE_DEVICE_BEAM", "1")
    dev_s = BeamOracleSession(model, 3)
    dev = TR.decode(model, first_window(dev_s, audio), session=dev_s, **opts)
    assert dev_s.calls["set_rules"] == 1 and dev_s.calls["kv_reorder"] == 0
    assert dev_s.calls["pick_topk"] == dev_s.calls["decode_ancestry"] + 1 > 1

    assert dev.tokens == host.tokens
    assert dev.tokens == want
    assert dev.avg_logprob == pytest.approx(host.avg_logprob, abs=1e-4)
    assert dev.no_speech_prob == host.no_speech_prob


@pytest.mark.parametrize("options", [dict(beam_size=8), dict(beam_size=3, temperature=0.4), dict(best_of=2, temperature=0.4),
                                     dict()])
def test_other_modes_keep_the_host_path_with_the_switch_on(options, real_vocab, monkeypatch):
    """Beam sizes outside 2..7, sampling and best_of never take the device beam branch."""
    monkeypatch.setenv("WLK_TRANSCRIBE_DEVICE_BEAM", "1")
    _, _, audio = beam_case()
    model = OracleModel("micro.en", 0)
    s = BeamOracleSession(model, options.get("beam_size") or options.get("best_of") or 1)
    TR.decode(model, first_window(s, audio), session=s, language="en", sample_len=3, **options)
    assert s.calls["pick_topk"] == 0 and s.calls["decode_ancestry"] == 0 and s.calls["set_rules"] == 0
