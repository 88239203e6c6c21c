"""Draft verification on the GPU (csrc/window_group.hip: wlk_group_verify; csrc/select.hip: draft_pick_rows_kernel,
draft_accept_kernel; whisperlivekit_amd/transcribe.py: the draft of decode / decode_many / transcribe): how much of a draft
greedy decoding would produce again, from ONE teacher-forced decoder pass.  Each window's truth is its stepwise decode
(wlk_decode + wlk_pick_greedy).

  1. every candidate position's pick is wlk_pick_greedy's, bit for bit, under the rule state of its history;
  2. `accepted` is the common prefix with the truth and `next_token` the truth's token there; log-probabilities within the
     allowance between the stacked and the solo route (5e-4 each, 5e-4 x (k + 1) for the sum);
  3. the smallest shapes (9, 32, 33, 64, 65 rows), with a prompt in front, and the no-speech probability;
  4. a window's results and what it leaves in its session do not depend on the windows beside it;
  5. the rejected tail of a draft leaves no trace in what follows;
  6. the session is what its own prefill of [initial | draft[:k]] leaves;
  7. decode / decode_many / transcribe give what they give without a draft;
  8. a call the host checks refuse has launched nothing and touched nobody.

The model is tiny.en, the smallest the stacked pass takes (micro.en is the model case 8 sees refused).  The windows are those
of tests/draft_verify_cases.py, whose decisions the CPU oracle keeps >= 1e-3 clear of a flip (tests/test_draft_verify_cpu.py),
so no comparison of token ids allows for ties."""
import threading

import numpy as np
import pytest

import draft_verify_cases as DV
import helpers as H
import window_burst_cases as WB
import window_group_cases as WG
from whisperlivekit_amd import _lib, synth, transcribe as TR

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -3


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


class _Runs:
    """tiny.en, one group of 8 rows, and the windows of draft_verify_cases each decoded step by step on its own session
    (wlk_decode + wlk_pick_greedy): computed once, read by every case."""

    def __init__(self, tmp_dir):
        from whisperlivekit_amd.engine import HipWhisperModel, HipWindowGroup
        self.mp = pytest.MonkeyPatch()
        self.mp.setenv("WLK_VOCAB_DIR", H.real_vocab_dir(tmp_dir))
        self.mp.setenv("WLK_SYNTHETIC_VOCAB", "0")
        for name in ("WLK_TRANSCRIBE_STACK", "WLK_TRANSCRIBE_STACK_BURST", "WLK_TRANSCRIBE_DRAFT"):
            self.mp.delenv(name, raising=False)
        self.model = HipWhisperModel.synthetic(DV.MODEL, DV.SEED, device=0)
        self.group = HipWindowGroup(self.model, 8)
        self.sessions, self.mels, self.spare = [], {}, {}
        self.truth = [self.stepwise(i) for i in range(len(DV.WINDOWS))]
        self.eot = self.truth[0].dec.tok.eot
        self.worst_lp, self.worst_sum, self.worst_ns = 0.0, 0.0, 0.0

    def session(self):
        s = self.model.new_session(beam=1, max_audio_seconds=1.0, batched=False)
        self.sessions.append(s)
        return s

    def encoded(self, index):
        """-> a window of WINDOWS[index] on a session of its own: encoded, rules set, nothing decoded"""
        w = DV.make_win(index, self.model, self.session())
        s = w.session
        if index not in self.mels:
            self.mels[index] = TR.pad_or_trim(s.log_mel(WG.window_audio(w.spec)))
        s.encode_mel(self.mels[index])
        s.set_rules(*w.rules())
        w.state0 = w.dec._pick_state(w.tokens)
        return w

    def lend(self, index):
        """an encoded window of WINDOWS[index] whose session a case may verify on (kept for the next case)"""
        if not self.spare.get(index):
            return self.encoded(index)
        return self.spare[index].pop()

    def give_back(self, w):
        self.spare.setdefault(w.index, []).append(w)

    def stepwise(self, index):
        w = self.encoded(index)
        s = w.session
        s.decode(w.tokens, first=True, sot_index=w.dec.sot_index)
        w.no_speech = float(s.no_speech_prob(w.dec.tok.no_speech)[0])
        w.rows, w.states = [], []
        while not w.over:
            state = w.dec._pick_state(w.tokens)
            w.rows.append(s.export("logits_last", self.model.dims.n_vocab).copy())
            w.states.append(state)
            w.take(*s.pick_greedy(**state))
            if not w.over:
                s.decode(w.tokens[:, -1:], first=False)
        return w

    def window(self, w, draft):
        return (w.session, list(w.dec.initial), [int(t) for t in draft], w.dec.sot_index, w.state0, w.dec.tok.no_speech)

    def check(self, index, res, draft):
        """a verify result against the truth of WINDOWS[index]; -> k"""
        t = self.truth[index]
        k, nxt, _lp, _sum = DV.expected(t.picks, draft, self.eot)
        assert (res["accepted"], res["next_token"]) == (k, nxt), (index, len(draft), res["accepted"], k)
        ids, lps = res["picks"]
        assert [int(x) for x in ids[:k + 1]] == [p[0] for p in t.picks[:k + 1]]
        want = np.asarray([p[1] for p in t.picks[:k + 1]], np.float32)
        diff = float(np.abs(lps[:k + 1] - want).max())
        total = np.float32(0.0)
        for v in want:
            total = np.float32(total + v)
        sum_diff = abs(float(res["sum_logprob"]) - float(total))
        ns_diff = abs(res["no_speech_prob"] - t.no_speech)
        self.worst_lp, self.worst_sum = max(self.worst_lp, diff), max(self.worst_sum, sum_diff / (k + 1))
        self.worst_ns = max(self.worst_ns, ns_diff)
        print(f"window {index} P0 {len(t.dec.initial)} n_d {len(draft)} k {k}: |dlp| {diff:.2e} |dsum| {sum_diff:.2e} |dns| {ns_diff:.2e}")
        assert diff <= DV.ALLOWANCE and sum_diff <= DV.ALLOWANCE * (k + 1) and ns_diff <= DV.ALLOWANCE
        assert bits(res["next_logprob"]) == bits(lps[k])
        # the sum is the device's own addends in the host loop's order
        got_sum = np.float32(0.0)
        for v in lps[:k + 1]:
            got_sum = np.float32(got_sum + v)
        assert bits(res["sum_logprob"]) == bits(got_sum)
        return k

    def close(self):
        TR.release_sessions(self.model)
        for s in self.sessions:
            s.close()
        self.group.close()
        self.model.close()
        self.mp.undo()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    r = _Runs(tmp_path_factory.mktemp("vocab"))
    yield r
    print(f"worst differences: log-probability {r.worst_lp:.3e}, sum per addend {r.worst_sum:.3e}, no-speech {r.worst_ns:.3e}")
    r.close()


def _kv(s, model):
    return [s.export(f"self_{kv}:{layer}") for layer in range(model.dims.n_text_layer) for kv in "kv"]


def _snapshot(w, model):
    return dict(logits=w.session.export("logits_last", model.dims.n_vocab).copy(), kv=_kv(w.session, model))


def _same_snapshot(a, b):
    assert np.array_equal(bits(a["logits"]), bits(b["logits"]))
    assert len(a["kv"]) == len(b["kv"])
    for x, y in zip(a["kv"], b["kv"]):
        assert x.shape == y.shape and np.array_equal(bits(x), bits(y))


def _continue(runs, w, res, draft, how):
    """the window goes on behind a verify pass for the rest of its sample_len: -> [(token, log-probability bits)] and the
    logits_last export after every call.  how: "group" (step_pick), "own" (wlk_decode + wlk_pick_greedy), "burst" (run_pick
    of 4)."""
    s, k = w.session, res["accepted"]
    w.tokens = np.asarray([list(w.dec.initial) + list(draft[:k]) + [res["next_token"]]], np.int64)
    out, logits = [], []
    left = w.spec["sample_len"] - (k + 1)
    while left > 0 and w.tokens[0, -1] != runs.eot:
        state = w.dec._pick_state(w.tokens)
        if how == "own":
            s.decode(w.tokens[:, -1:], first=False)
            tok, lp = s.pick_greedy(**state)
            ids, lps = [tok], [lp]
            logits.append(s.export("logits_last", runs.model.dims.n_vocab).copy())
        elif how == "group":
            ids, lps = runs.group.step_pick([s], [int(w.tokens[0, -1])], [state])
            logits.append(runs.group.export_logits(0).copy())
        else:
            (ids, lps), = runs.group.run_pick([s], [int(w.tokens[0, -1])], [state], [left], 4)
            logits.append(runs.group.export_logits(0).copy())
        for t, lp in zip(ids, lps):
            out.append((int(t), int(bits(lp))))
            w.tokens = np.concatenate([w.tokens, np.asarray([[int(t)]], np.int64)], axis=1)
            left -= 1
    return out, logits


# ---- 1. the pick of every candidate position -----------------------------------------------------------------------------------
def test_every_position_picks_what_pick_greedy_picks_bit_for_bit(runs):
    from whisperlivekit_amd.engine import draft_pick, pick_rows
    V = runs.model.dims.n_vocab
    walked = set()
    # the logits rows, rule states and picks of the stepwise decodes: wlk_pick_greedy itself is the reference
    for index in (0, 2, 1):
        t = runs.truth[index]
        n = min(len(t.picks), 40)
        draft = [p[0] for p in t.picks[:n - 1]]
        mask = WG.rules_mask(V, *t.rules())
        ids, lps, res = draft_pick(np.stack(t.rows[:n]), mask, t.states[0], draft)
        assert [int(x) for x in ids] == [p[0] for p in t.picks[:n]]
        assert np.array_equal(bits(lps), bits([p[1] for p in t.picks[:n]]))
        assert res["accepted"] == n - 1 and res["next_token"] == t.picks[n - 1][0]
        walked |= {(a["ts_mode"], b["ts_mode"]) for a, b in zip(t.states[:n - 1], t.states[1:n]) if not a["without_timestamps"]}
    assert {(0, 1), (1, 0), (0, 2), (2, 1)} <= walked, walked
    # histories that walk every branch of the timestamp rules, random logits, two suppress lists: the rows pick (bit-identical
    # to wlk_pick_greedy by its own contract) under the HOST's state of each prefix
    rng = np.random.default_rng(11)
    decs = [TR._WindowDecoder(runs.model, TR.DecodingOptions(language="en", temperature=0.0, suppress_tokens=sup,
                                                             without_timestamps=flag))
            for sup, flag in ((f"-1,{runs.eot}", False), ("-1", True), ("300,301,5000", False))]
    for dec in decs:
        mask = WG.rules_mask(V, dec.suppressed or [], dec.blank_ids or [])
        for h in WB.histories(dec, rng):
            h = [t for t in h if t != runs.eot]
            if not h:
                continue
            logits = (rng.standard_normal((len(h) + 1, V)) * 3.0).astype(np.float32)
            states = [WB.state_of(dec, h[:j]) for j in range(len(h) + 1)]
            ids, lps, res = draft_pick(logits, mask, states[0], h)
            want_ids, want_lps = pick_rows(logits, mask[None, :], [0] * len(states), states)
            assert np.array_equal(ids, want_ids) and np.array_equal(bits(lps), bits(want_lps)), h
            k, nxt, lp, total = TR._accept_draft(list(zip(ids, lps)), h, runs.eot)
            assert (res["accepted"], res["next_token"]) == (k, nxt)
            assert bits(res["next_logprob"]) == bits(lp) and bits(res["sum_logprob"]) == bits(total)
    # a long draft: more than one ballot round, the mismatch in the last one
    n = 200
    logits = (rng.standard_normal((n + 1, V)) * 3.0).astype(np.float32)
    dec = decs[1]
    mask = WG.rules_mask(V, dec.suppressed or [], dec.blank_ids or [])
    state = WB.state_of(dec, [])
    ids, _lps, _res = draft_pick(logits, mask, state, [400] * n)
    draft = [int(t) for t in ids[:n]]
    for at in (None, 199, 130, 64, 63, 0):
        d = list(draft) if at is None else DV.spoiled(draft, at)
        ids2, lps2, res = draft_pick(logits, mask, state, d)
        k, nxt, lp, total = TR._accept_draft(list(zip(ids2, lps2)), d, runs.eot)
        assert k == (n if at is None else at) and (res["accepted"], res["next_token"]) == (k, nxt)
        assert bits(res["sum_logprob"]) == bits(total)
    assert draft_pick(logits[:3], mask, state, draft[:2], ended=True)[2]["accepted"] == 0


# ---- 2. acceptance ----------------------------------------------------------------------------------------------------------------
def test_accepted_is_the_common_prefix_with_the_stepwise_decode(runs):
    t = runs.truth[0]
    truth = DV.sampled(t.picks, runs.eot)
    assert len(t.dec.initial) == 1 and len(truth) == 66
    drafts = [truth[:65], DV.spoiled(truth[:40], 0), DV.spoiled(truth[:40], 1), DV.spoiled(truth[:40], 30),
              DV.spoiled(truth[:40], 31), DV.spoiled(truth[:40], 32), DV.spoiled(truth[:40], 39)]
    w = runs.lend(0)
    ks = []
    for draft in drafts:
        res, = runs.group.verify([runs.window(w, draft)], want_picks=True)
        ks.append(runs.check(0, res, draft))
    assert ks == [65, 0, 1, 30, 31, 32, 39]                   # P0 + k at 31, 32 and 33 among them
    runs.give_back(w)
    # the window that ends: its whole truth, and the truth with tokens behind its end - the pick there is <|endoftext|>
    e = runs.truth[DV.EOT_WINDOW]
    sampled = DV.sampled(e.picks, runs.eot)
    assert e.picks[-1][0] == runs.eot and len(sampled) == len(e.picks) - 1 >= 1
    w = runs.lend(DV.EOT_WINDOW)
    for draft in (sampled, sampled + [500, 501, 502]):
        res, = runs.group.verify([runs.window(w, draft)], want_picks=True)
        assert runs.check(DV.EOT_WINDOW, res, draft) == len(sampled) and res["next_token"] == runs.eot
    runs.give_back(w)
    # without timestamps
    t1 = DV.sampled(runs.truth[1].picks, runs.eot)
    w = runs.lend(1)
    for draft in (t1[:23], DV.spoiled(t1[:23], 11)):
        res, = runs.group.verify([runs.window(w, draft)], want_picks=True)
        runs.check(1, res, draft)
    runs.give_back(w)


# ---- 3. the smallest shapes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [9, 32, 33, 64, 65])
def test_the_smallest_shapes_with_a_prompt_in_front(runs, rows):
    for index in (0, DV.PROMPT_WINDOW):
        t = runs.truth[index]
        p0 = len(t.dec.initial)
        truth = DV.sampled(t.picks, runs.eot)
        assert runs.group.verify_fits(p0, rows - p0) and (index == 0 or t.dec.sot_index == 6)
        w = runs.lend(index)
        for draft in (truth[:rows - p0], DV.spoiled(truth[:rows - p0], rows - p0 - 2)):
            assert len(draft) == rows - p0
            res, = runs.group.verify([runs.window(w, draft)], want_picks=True)
            runs.check(index, res, draft)
            # what wlk_no_speech_prob and wlk_pick_greedy say afterwards: the session's own calls on the rows the pass left
            assert abs(float(w.session.no_speech_prob(t.dec.tok.no_speech)[0]) - t.no_speech) <= DV.ALLOWANCE
            k = res["accepted"]
            tok, lp = w.session.pick_greedy(**t.states[k])
            assert tok == res["next_token"] and bits(lp) == bits(res["next_logprob"])
        runs.give_back(w)
    assert not runs.group.verify_fits(1, 7) and not runs.group.verify_fits(2, 6) and runs.group.verify_fits(8, 1)
    assert runs.group.verify_fits(1, 255) and not runs.group.verify_fits(1, 256) and not runs.group.verify_fits(0, 20)
    assert not runs.group.verify_fits(5, 0)


# ---- 4. neighbours ------------------------------------------------------------------------------------------------------------------
def test_a_windows_results_do_not_depend_on_the_windows_beside_it(runs):
    truths = [DV.sampled(t.picks, runs.eot) for t in runs.truth]
    # (window, draft): different P and different k
    plan = [(0, truths[0][:65]), (1, DV.spoiled(truths[1][:23], 5)), (2, truths[2][:26]), (3, truths[3] + [500, 501]),
            (4, DV.spoiled(truths[4][:29], 28)), (0, DV.spoiled(truths[0][:31], 0)), (2, DV.spoiled(truths[2][:57], 40)),
            (4, truths[4][:8])]
    wins = [runs.lend(i) for i, _d in plan]
    alone = []
    for w, (_i, draft) in zip(wins, plan):
        res, = runs.group.verify([runs.window(w, draft)], want_picks=True)
        alone.append((res, _snapshot(w, runs.model)))
    assert len({len(w.dec.initial) + len(d) for w, (_i, d) in zip(wins, plan)}) >= 7
    assert len({a[0]["accepted"] for a in alone}) >= 6
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 5, 8):
        order = [int(i) for i in rng.permutation(8)[:n]]
        got = runs.group.verify([runs.window(wins[i], plan[i][1]) for i in order], want_picks=True)
        for i, res in zip(order, got):
            want, snap = alone[i]
            for key in ("accepted", "next_token"):
                assert res[key] == want[key], (n, i, key)
            for key in ("next_logprob", "sum_logprob", "no_speech_prob"):
                assert bits(res[key]) == bits(want[key]), (n, i, key)
            assert np.array_equal(res["picks"][0], want["picks"][0]) and np.array_equal(bits(res["picks"][1]), bits(want["picks"][1]))
            _same_snapshot(_snapshot(wins[i], runs.model), snap)
    for w in wins:
        runs.give_back(w)


# ---- 5. the rejected tail ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["group", "own", "burst"])
def test_the_rejected_tail_leaves_no_trace(runs, how):
    t = runs.truth[4]
    truth = DV.sampled(t.picks, runs.eot)
    k = 12
    # both passes project more than 8 rows onto the vocabulary (the projection's kernel is chosen by the row count)
    tail = truth[:k] + [DV.wrong(truth[k])] + [int(x) for x in np.random.default_rng(2).integers(300, 20000, 9)]
    full = truth[:k]
    a, b = runs.lend(4), runs.lend(4)
    ra, = runs.group.verify([runs.window(a, tail)])
    rb, = runs.group.verify([runs.window(b, full)])
    assert ra["accepted"] == rb["accepted"] == k and ra["next_token"] == rb["next_token"] == t.picks[k][0]
    assert bits(ra["next_logprob"]) == bits(rb["next_logprob"]) and bits(ra["sum_logprob"]) == bits(rb["sum_logprob"])
    _same_snapshot(_snapshot(a, runs.model), _snapshot(b, runs.model))
    out_a, logits_a = _continue(runs, a, ra, tail, how)
    out_b, logits_b = _continue(runs, b, rb, full, how)
    assert out_a == out_b and len(out_a) == t.spec["sample_len"] - (k + 1)
    assert [p[0] for p in out_a] == [p[0] for p in t.picks[k + 1:]]              # and it is the truth's continuation
    assert len(logits_a) == len(logits_b) and all(np.array_equal(bits(x), bits(y)) for x, y in zip(logits_a, logits_b))
    for x, y in zip(_kv(a.session, runs.model), _kv(b.session, runs.model)):
        assert x.shape == y.shape and np.array_equal(bits(x), bits(y))
    runs.give_back(a)
    runs.give_back(b)


# ---- 6. against a prefill --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index,n_draft,at", [(0, 40, 30), (2, 30, 9), (1, 23, None)])
def test_the_session_is_what_its_own_prefill_of_the_accepted_tokens_leaves(runs, index, n_draft, at):
    t = runs.truth[index]
    truth = DV.sampled(t.picks, runs.eot)
    draft = truth[:n_draft] if at is None else DV.spoiled(truth[:n_draft], at)
    a, b = runs.lend(index), runs.lend(index)
    res, = runs.group.verify([runs.window(a, draft)])
    k = res["accepted"]
    assert k == (n_draft if at is None else at) and 9 <= len(t.dec.initial) + k <= 256
    prompt = np.asarray([list(t.dec.initial) + draft[:k]], np.int64)
    b.session.decode(prompt, first=True, sot_index=t.dec.sot_index)
    tok, lp = b.session.pick_greedy(**t.states[k])
    assert tok == res["next_token"] and abs(lp - float(res["next_logprob"])) <= DV.ALLOWANCE
    for x, y in zip(_kv(a.session, runs.model), _kv(b.session, runs.model)):
        assert x.shape == y.shape and x.size == prompt.shape[1] * runs.model.dims.n_text_state
        assert np.array_equal(bits(x), bits(y))
    rb = dict(accepted=k, next_token=tok)
    out_a, logits_a = _continue(runs, a, res, draft, "group")
    out_b, logits_b = _continue(runs, b, rb, draft, "group")
    assert out_a == out_b and all(np.array_equal(bits(x), bits(y)) for x, y in zip(logits_a, logits_b))
    for x, y in zip(_kv(a.session, runs.model), _kv(b.session, runs.model)):
        assert np.array_equal(bits(x), bits(y))
    runs.give_back(a)
    runs.give_back(b)


# ---- 7. end to end -----------------------------------------------------------------------------------------------------------------------
OPTS = dict(language="en", temperature=0.0, sample_len=24)


def _close(got, want):
    assert got.tokens == want.tokens and got.text == want.text and got.temperature == want.temperature
    assert abs(got.avg_logprob - want.avg_logprob) <= DV.ALLOWANCE
    assert abs(got.no_speech_prob - want.no_speech_prob) <= DV.ALLOWANCE and got.compression_ratio == want.compression_ratio


def test_decode_and_decode_many_with_drafts_give_what_they_give_without(runs):
    model = runs.model
    eot = runs.eot
    opts = TR.DecodingOptions(**OPTS, suppress_tokens=f"-1,{eot}")
    stacker = TR.WindowStacker(model, 8, group=runs.group)
    mels = [runs.mels[i] for i in (0, 4, 2)]
    want = [TR.decode(model, m, opts, stacker=stacker) for m in mels]
    assert all(len(w.tokens) == 24 for w in want)
    for draft in (want[0].tokens, DV.spoiled(want[0].tokens, 10), want[0].tokens[:8] + [5000] * 30, [], [eot]):
        _close(TR.decode(model, mels[0], replace_draft(opts, draft), stacker=stacker), want[0])
    got = TR.decode_many(model, mels, opts, stacker=stacker, drafts=[want[0].tokens, None, DV.spoiled(want[2].tokens, 3)])
    for g, w in zip(got, want):
        _close(g, w)
    TR.release_sessions(model)


def replace_draft(opts, draft):
    from dataclasses import replace
    return replace(opts, draft=draft)


KW = dict(language="en", temperature=0.0, sample_len=24, without_timestamps=True, logprob_threshold=None, compression_ratio_threshold=None,
          no_speech_threshold=None, word_timestamps=True)


def _same_transcript(got, want):
    assert got["text"] == want["text"] and len(got["segments"]) == len(want["segments"])
    for g, w in zip(got["segments"], want["segments"]):
        assert g["tokens"] == w["tokens"] and (g["start"], g["end"], g["seek"]) == (w["start"], w["end"], w["seek"])
        assert abs(g["avg_logprob"] - w["avg_logprob"]) <= DV.ALLOWANCE and abs(g["no_speech_prob"] - w["no_speech_prob"]) <= DV.ALLOWANCE
        assert [(x["word"], x["start"], x["end"]) for x in g["words"]] == [(x["word"], x["start"], x["end"]) for x in w["words"]]


def test_transcribe_on_a_growing_buffer_through_a_session_view(runs):
    from whisperlivekit_amd.local_agreement import HipWhisperASR
    model = runs.model
    audio = synth.speech_like(8.0, seed=5)
    kw = {k: v for k, v in KW.items() if k not in ("language", "word_timestamps")}
    kw["suppress_tokens"] = f"-1,{runs.eot}"
    try:
        off = HipWhisperASR("en", hip_model=model, stack=8)
        off.transcribe_kargs = dict(kw)
        ends = [int(16000 * s) for s in (6.0, 6.5, 7.0)]
        want = [off.transcribe(audio[:e]) for e in ends]
        trimmed = off.transcribe(audio[16000:ends[2] + 8000])
        on = HipWhisperASR("en", hip_model=model, stack=8, draft=True)
        on.transcribe_kargs = dict(kw)
        view = on.session_view()
        for e, w in zip(ends, want):
            _same_transcript(view.transcribe(audio[:e]), w)
        assert view.memory.offered == 2 and view.memory.dropped == 0
        _same_transcript(view.transcribe(audio[16000:ends[2] + 8000]), trimmed)      # the buffer was trimmed: no draft
        assert view.memory.offered == 2 and view.memory.dropped == 1
        # four threads with a view each
        views = [on.session_view() for _ in range(4)]
        got, errors = [None] * 4, []

        def work(i):
            try:
                got[i] = [views[i].transcribe(audio[:e]) for e in ends]
            except BaseException as e:               # noqa: BLE001 - reported below
                errors.append(e)
        threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for i in range(4):
            assert views[i].memory.offered == 2
            for g, w in zip(got[i], want):
                _same_transcript(g, w)
    finally:
        TR.set_stack(model, 0)
        st = model.__dict__.pop("_window_stacker", None)
        if st is not None:
            st.close()
        TR.release_sessions(model)


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------
def test_a_refused_call_has_launched_nothing_and_touched_nobody(runs):
    from whisperlivekit_amd.engine import HipWhisperModel, HipWindowGroup
    model, group = runs.model, runs.group
    t = runs.truth[4]
    truth = DV.sampled(t.picks, runs.eot)
    k = 9
    good, twin, other = runs.lend(4), runs.lend(4), runs.lend(0)
    states = []
    for w in (good, twin):                                     # both in the middle of a window: prefilled and one step in
        w.session.decode(np.asarray([list(w.dec.initial) + truth[:k]], np.int64), first=True, sot_index=w.dec.sot_index)
        states.append(t.states[k])
    plain = runs.window(other, DV.sampled(runs.truth[0].picks, runs.eot)[:20])
    g = runs.window(good, truth[:20])

    def refused(windows, code, grp=None):
        with pytest.raises(_lib.WlkError) as e:
            (grp or group).verify(windows)
        assert e.value.code == code, (e.value, code)

    def with_(win, **kw):
        s, initial, draft, sot, state, ns = win
        d = dict(s=s, initial=initial, draft=draft, sot=sot, state=state, ns=ns)
        d.update(kw)
        return (d["s"], d["initial"], d["draft"], d["sot"], d["state"], d["ns"])
    refused([], ERR_ARG)
    refused([plain, g, g], ERR_ARG)                                                  # a session listed twice
    refused([plain, with_(g, draft=[])], ERR_ARG)                                    # an empty draft
    refused([plain, with_(g, draft=truth[:5] + [runs.eot] + truth[6:20])], ERR_ARG)  # <|endoftext|> in the draft
    refused([plain, with_(g, draft=truth[:5] + [model.dims.n_vocab])], ERR_ARG)      # a token out of range
    refused([plain, with_(g, draft=truth[:7])], ERR_ARG)                             # 8 rows: below the stacked range
    refused([plain, with_(g, draft=[400] * 256)], ERR_ARG)                           # 257 rows
    refused([plain, with_(g, initial=[])], ERR_ARG)
    refused([plain, with_(g, sot=1)], ERR_ARG)                                       # sot_index outside the initial tokens
    refused([plain, with_(g, state=dict(g[4], ts_mode=3))], ERR_ARG)
    refused([plain, with_(g, ns=model.dims.n_vocab)], ERR_ARG)
    bare = runs.session()
    refused([plain, with_(g, s=bare)], ERR_STATE)                                    # not encoded
    bare.encode_mel(runs.mels[4])
    refused([plain, with_(g, s=bare)], ERR_STATE)                                    # no rules
    beams = model.new_session(beam=2, max_audio_seconds=1.0, batched=False)
    runs.sessions.append(beams)
    refused([plain, with_(g, s=beams)], ERR_ARG)
    small = HipWindowGroup(model, 1)
    refused([plain, g], ERR_ARG, small)                                              # more windows than the group's rows
    small.close()
    # a model the stacked pass does not take, and a session of another model
    micro = HipWhisperModel.synthetic(DV.REFUSED_MODEL, 3, device=0)
    try:
        mg = HipWindowGroup(micro, 8)
        assert not any(mg.verify_fits(1, n) for n in (8, 31, 100, 255))
        ms = micro.new_session(beam=1, max_audio_seconds=1.0, batched=False)
        ms.encode_mel(runs.mels[4])
        ms.set_rules(*good.rules())
        refused([with_(g, s=ms)], ERR_ARG, mg)
        refused([plain, with_(g, s=ms)], ERR_ARG)
        # ... and decode() with a draft on that model takes the prefill, as without one
        opts = TR.DecodingOptions(language="en", temperature=0.0, sample_len=12, suppress_tokens=f"-1,{runs.eot}")
        st = TR.WindowStacker(micro, 8, group=mg)
        want = TR.decode(micro, runs.mels[4], opts, stacker=st)
        assert TR.decode(micro, runs.mels[4], replace_draft(opts, want.tokens), stacker=st) == want
        TR.release_sessions(micro)
        ms.close()
        mg.close()
    finally:
        micro.close()
    # every refused call left `good` where it was: it goes on to the bits of the twin that never met one
    out = []
    for w, state in zip((good, twin), states):
        tok, lp = w.session.pick_greedy(**state)
        res = dict(accepted=k, next_token=tok)
        steps, logits = _continue(runs, w, res, truth, "group")
        out.append(((tok, int(bits(lp))), steps, logits, _kv(w.session, model)))
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1] and out[0][0][0] == t.picks[k][0]
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(out[0][2], out[1][2]))
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(out[0][3], out[1][3]))
    # and `other`, listed first in every refused call, was never touched: its first verify is a window's first
    res, = group.verify([plain], want_picks=True)
    runs.check(0, res, plain[2])
    for w in (good, twin, other):
        runs.give_back(w)
