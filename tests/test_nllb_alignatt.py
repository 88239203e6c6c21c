"""AlignAtt streaming translation on the CPU: the stand-in session against `transformers`' own
cross-attention (tests/golden/nllb_align_kat.npz, scripts/gen_golden_nllb_align.py), the rule of
`nllb.generate_alignatt` against the stored outcomes, and the session object `HipAlignAttTranslation` over a scripted
model.  The gpu-marked twins (tests/test_gpu_nllb_alignatt.py) run the library."""
import os
import re
import types

import numpy as np
import pytest

import helpers as H
import nllb_align_standin as A
from nllb_align_standin import AlignOracleNllbSession, align_gain_state_dict, readout
from oracle.nllb_oracle import NllbOracle
from whisperlivekit_amd import _lib, nllb
from whisperlivekit_amd import translation as T
from whisperlivekit_amd.policy import ASRToken

KAT = H.golden_npz("nllb_align_kat.npz")
N_CASES = int(KAT["n_cases"])
CFG = nllb.NLLB_MICRO
P_ATOL = 5e-5          # the bound tests/test_nllb.py gives the oracle against transformers


def settings_of(prefix):
    return A.settings_of(KAT, prefix)


@pytest.fixture(scope="module")
def micro_oracle():
    return NllbOracle(CFG, align_gain_state_dict(CFG, 0))


def follow_greedy(sess, prefix, atol):
    return A.follow_greedy(sess, KAT, prefix, atol)


def test_fixture_holds_what_the_tests_rely_on():
    gaps = np.concatenate([KAT[f"c{ci}_gap"] for ci in range(N_CASES)])
    assert gaps.min() > 4e-4                                   # no step of a micro case needs exempting
    open_runs = [(len(ids), why) for ci in range(N_CASES) for _k, _n, _t, final, _c, _m, ids, _a, why in settings_of(f"c{ci}_")
                 if not final]
    assert any(n == 0 and why == "attention" for n, why in open_runs)
    assert any(n >= 3 and why == "attention" for n, why in open_runs)
    assert any(n > 0 and why == "length" for n, why in open_runs)
    assert float(KAT["big_gap"].min()) > 2e-3
    for ci in range(N_CASES):
        assert float(np.abs(KAT[f"c{ci}_p32"] - KAT[f"c{ci}_p64"]).max()) < 5e-6


@pytest.mark.parametrize("ci", range(N_CASES))
def test_standin_matches_transformers(micro_oracle, ci):
    sess = AlignOracleNllbSession(micro_oracle, 1)
    sess.set_alignment_heads(KAT["heads"].tolist())
    assert [tuple(h) for h in KAT["heads"].tolist()] == nllb.default_alignment_heads(CFG)
    follow_greedy(sess, f"c{ci}_", P_ATOL)


def test_standin_matches_transformers_at_the_600m_shape():
    cfg = nllb.NLLB_200_DISTILLED_600M
    import torch
    torch.set_num_threads(8)
    sess = AlignOracleNllbSession(NllbOracle(cfg, align_gain_state_dict(cfg, int(KAT["big_seed"]))), 1)
    sess.set_alignment_heads(KAT["big_heads"].tolist())
    assert [tuple(h) for h in KAT["big_heads"].tolist()] == nllb.default_alignment_heads(cfg)
    follow_greedy(sess, "big_", P_ATOL)


@pytest.mark.parametrize("ci", range(N_CASES))
def test_generate_alignatt_over_the_standin_reproduces_the_stored_outcomes(micro_oracle, ci):
    prefix = f"c{ci}_"
    sess = AlignOracleNllbSession(micro_oracle, 1)
    sess.set_alignment_heads(KAT["heads"].tolist())
    for k, n_acc, thr, final, committed, max_new, want_ids, want_align, want_why in settings_of(prefix):
        got = nllb.generate_alignatt(sess, KAT[prefix + "src"], int(KAT[prefix + "lang"]), committed=committed, n_accessible=n_acc,
                                     threshold=thr, final=final, max_new_tokens=max_new, device_loop=False)
        assert got == (want_ids, want_align, want_why), f"setting {k}: {(n_acc, thr, final, len(committed), max_new)}"


def test_readout_restatement_rules():
    """the stand-in's read-out: rank-order sum x float32(1 / n), lowest position on a tie, -1 on an empty window"""
    probs = np.zeros((3, 1, 6), np.float32)
    probs[:, 0, 2] = probs[:, 0, 4] = 0.25
    probs[:, 0, 0] = 0.5
    p, pos, prob, mass = readout(probs, 1, 5, 3)
    assert pos[0] == 2 and prob[0] == p[0, 2] and mass[0] == p[0, 3:].sum(dtype=np.float32)
    assert readout(probs, 0, 6, 0)[1][0] == 0 and readout(probs, 3, 3, 0)[1][0] == -1 and readout(probs, 4, 2, 6)[3][0] == 0


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wlk_hip.h")).read()
    declared = set(re.findall(r"\b(wlk_[a-z_0-9]+)\s*\(", header))
    for name in ("wlk_nllb_session_set_align", "wlk_nllb_step_align", "wlk_nllb_generate_alignatt", "wlk_nllb_session_align_stats",
                 "wlk_diag_nllb_align"):
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), name), name


# ---- the rule over a scripted session ----------------------------------------------------------------------------------
LANGS = {"eng_Latn": 1990, "fra_Latn": 1991}
EOS = CFG.eos_token_id


class ScriptedSession:
    """A 'translation' that copies: target token t is content id t + 1000 and leans on source position 1 + t; behind the
    content comes </s>, leaning on the last content position.  Counts its steps."""

    def __init__(self, lookahead=0):
        self.rows, self.model = 1, types.SimpleNamespace(cfg=CFG)
        self.lookahead = lookahead                 # how far ahead of its own word a token looks
        self.heads, self.steps, self.encodes, self.fed = None, 0, 0, []

    def set_alignment_heads(self, pairs):
        self.heads = list(pairs)

    def encode(self, src):
        self.src, self.encodes = [int(v) for v in src], self.encodes + 1

    def decode(self, tokens, first):
        assert first
        self.fed = [int(t) for t in np.asarray(tokens).reshape(-1)]

    def step_align(self, tokens, k, lo, hi, limit):
        self.fed.append(int(tokens[0]))
        self.steps += 1
        t = len(self.fed) - 2                      # tokens behind [</s>, language]
        content = self.src[1:-1]
        y = content[t] + 1000 if t < len(content) else EOS
        a = min(1 + t + self.lookahead, len(self.src) - 2)
        a = a if lo <= a < hi else -1
        return np.zeros((1, 1), np.float32), np.asarray([[y]], np.int32), np.asarray([a], np.int32), None, None

    def close(self):
        pass


def test_rule_on_a_scripted_session():
    src = [1990, 10, 11, 12, 13, 14, EOS]
    run = lambda **kw: nllb.generate_alignatt(ScriptedSession(), src, 1991, device_loop=False, **kw)     # noqa: E731
    assert run(n_accessible=6, threshold=2, final=False) == ([1010, 1011, 1012], [1, 2, 3], "attention")
    assert run(n_accessible=6, threshold=0, final=False) == ([1010, 1011, 1012, 1013, 1014], [1, 2, 3, 4, 5], "eos")
    assert run(n_accessible=6, threshold=0, final=True) == ([1010, 1011, 1012, 1013, 1014], [1, 2, 3, 4, 5], "eos")
    assert run(n_accessible=3, threshold=9, final=False) == ([], [], "attention")          # a limit below lo counts as lo
    assert run(n_accessible=6, threshold=0, final=False, max_new_tokens=2) == ([1010, 1011], [1, 2], "length")
    assert run(n_accessible=6, threshold=0, final=False, max_new_tokens=0) == ([], [], "length")
    assert run(n_accessible=2, threshold=0, final=True, committed=[1010, 1011]) == ([1012, 1013, 1014], [3, 4, 5], "eos")
    assert run(n_accessible=6, threshold=1, final=False, committed=[1010, 1011]) == ([1012, 1013], [3, 4], "attention")
    assert nllb.generate_alignatt(ScriptedSession(), [1990, EOS], 1991, n_accessible=1, threshold=0, final=False,
                                  device_loop=False) == ([], [], "attention")               # empty window: position -1
    with pytest.raises(ValueError):
        run(n_accessible=8, threshold=0, final=False)


# ---- the session object -----------------------------------------------------------------------------------------------
class WordTokenizer:
    """one id per word: [language code] words </s>; `merge` joins the named adjacent pair into one id (a tokenizer that
    merges across the committed / tail boundary)"""
    unk_token_id = 3

    def __init__(self, merge=None):
        self.src_lang, self.merge = "eng_Latn", merge

    @staticmethod
    def _id(w):
        h = 0
        for ch in w:
            h = (h * 131 + ord(ch)) % 900
        return 10 + h

    def __call__(self, text):
        ws = text.lower().split()
        if self.merge:
            i = 0
            while i + 1 < len(ws):
                if (ws[i], ws[i + 1]) == self.merge:
                    ws[i:i + 2] = [ws[i] + ws[i + 1]]
                i += 1
        return types.SimpleNamespace(input_ids=[LANGS[self.src_lang]] + [self._id(w) for w in ws] + [EOS])

    def convert_tokens_to_ids(self, tok):
        return LANGS.get(tok, self.unk_token_id)

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(f"w{int(i)}" for i in ids)


class ScriptedModel:
    cfg = CFG

    def __init__(self, lookahead=0):
        self.lookahead, self.sessions = lookahead, []

    def new_session(self, rows=1):
        self.sessions.append(ScriptedSession(self.lookahead))
        return self.sessions[-1]


Tail = A.HypothesisTail


def words(spec, t0=0.0):
    return [ASRToken(start=round(t0 + 0.4 * i, 2), end=round(t0 + 0.4 * i + 0.4, 2), text=" " + w) for i, w in enumerate(spec.split())]


def make(threshold=1, tail=False, merge=None, lookahead=0, clock=None):
    tm = T.HipNllbTranslationModel(ScriptedModel(lookahead), WordTokenizer(merge), policy="alignatt", threshold=threshold,
                                   hypothesis_tail=tail)
    tr = tm.new_session("eng_Latn", "fra_Latn")
    if clock is not None:
        tr._clock = clock
    return tm, tr


def test_policy_selects_the_session_class():
    tm, tr = make()
    assert isinstance(tr, T.HipAlignAttTranslation) and tr.wants_hypothesis_tail is False
    assert tr.session.heads == nllb.default_alignment_heads(CFG)
    assert isinstance(T.online_translation_factory(tm, "eng_Latn", "fra_Latn"), T.HipAlignAttTranslation)
    heads = T.HipNllbTranslationModel(ScriptedModel(), WordTokenizer(), policy="alignatt", alignment_heads=[(0, 1)])
    assert heads.new_session("eng_Latn", "fra_Latn").session.heads == [(0, 1)]
    from oracle.nllb_oracle import OracleNllbSession
    oracle_model = types.SimpleNamespace(cfg=CFG, new_session=lambda rows=1: OracleNllbSession(types.SimpleNamespace(cfg=CFG), rows))
    default = T.HipNllbTranslationModel(oracle_model, WordTokenizer())
    assert default.policy == "local_agreement" and type(default.new_session("eng_Latn", "fra_Latn")) is T.HipOnlineTranslation
    assert type(T.online_translation_factory(default, "eng_Latn", "fra_Latn")) is T.HipOnlineTranslation
    with pytest.raises(ValueError):
        T.HipNllbTranslationModel(ScriptedModel(), WordTokenizer(), policy="wait_k")
    with pytest.raises(ValueError):
        T.HipNllbTranslationModel(ScriptedModel(), WordTokenizer(), policy="alignatt", num_beams=2)


def test_unknown_target_language_falls_back():
    tm, _ = make()
    with pytest.raises(ValueError):
        tm.new_session("eng_Latn", "xxx_Latn")
    tr = T.online_translation_factory(tm, "eng_Latn", "xxx_Latn", fallback_target="fra_Latn")
    assert isinstance(tr, T.HipAlignAttTranslation) and tr.target_language == "fra_Latn"
    with pytest.raises(ValueError):
        T.online_translation_factory(tm, "eng_Latn", "xxx_Latn")


def test_text_on_screen_only_grows_within_a_sentence_and_finals_come_one_per_call():
    tm, tr = make(threshold=1)
    tok = WordTokenizer()
    sentence = "the quick brown fox jumps over the lazy dog."
    shown = ""
    for i, w in enumerate(words(sentence)[:-1]):
        tr.insert_tokens([w])
        new, buf = tr.process()
        assert new is None and isinstance(buf, T.TimedText)
        assert (buf.text or "").startswith(shown), (shown, buf.text)
        shown = buf.text or ""
        # the copy model leans on its own word: all but the newest `threshold` words are out
        assert len(shown.split()) == max(i + 1 - 1, 0)
    assert shown
    # the sentence ends, and two more arrive in the same batch of tokens
    tr.insert_tokens(words(sentence, 0.0)[-1:] + words("second one.", 4.0) + words("third", 5.0))
    want = " ".join(f"w{i + 1000}" for i in tok(sentence).input_ids[1:-1])
    new, buf = tr.process()
    assert isinstance(new, T.Translation) and new.text == want and new.text.startswith(shown)
    assert (new.start, new.end) == (0.0, 3.6)
    new2, buf2 = tr.process()
    assert new2.text == " ".join(f"w{i + 1000}" for i in tok("second one.").input_ids[1:-1]) and (new2.start, new2.end) == (3.6, 4.8)
    new3, buf3 = tr.process()                              # the open sentence: one word, held back by the threshold
    assert new3 is None and not buf3.text
    assert tr.finals == 2


def test_silence_or_speaker_change_validates_the_screen_and_starts_afresh():
    tm, tr = make(threshold=1)
    tr.insert_tokens(words("one two three four"))
    _, buf = tr.process()
    assert buf.text == "w%d w%d w%d" % tuple(WordTokenizer._id(w) + 1000 for w in ("one", "two", "three"))
    validated, empty = tr.validate_buffer_and_reset()
    assert isinstance(validated, T.Translation) and validated.text == buf.text and (validated.start, validated.end) == (0.0, 1.6)
    assert isinstance(empty, T.TimedText) and not empty.text
    tr.insert_silence(2.5)
    assert tr._silence == 2.5
    # the queued final pass hands out only what lies behind the validated text
    new, buf = tr.process()
    assert new.text == "w%d" % (WordTokenizer._id("four") + 1000) and new.start == 1.6
    tr.insert_tokens(words("fresh start here", 5.0))
    new, buf = tr.process()
    assert new is None and buf.text.split()[0] == "w%d" % (WordTokenizer._id("fresh") + 1000) and buf.start == 1.6
    nothing, _ = T.HipNllbTranslationModel(ScriptedModel(), WordTokenizer(), policy="alignatt").new_session(
        "eng_Latn", "fra_Latn").validate_buffer_and_reset()
    assert isinstance(nothing, T.Translation) and nothing.text == ""


def test_tail_updates_follow_the_injected_clock():
    now = [100.0]
    tm, tr = make(threshold=0, tail=True, clock=lambda: now[0])
    assert tr.wants_hypothesis_tail is True
    sess = tr.session
    tr.insert_tokens(words("alpha beta"))
    tr.process()
    assert sess.encodes == 1 and len(sess.src) == 4
    tr.insert_tokens([Tail("gamma")])
    tr.process()                                           # a tail-only change, 0 s after the last run: not yet
    assert sess.encodes == 1
    now[0] += 0.49
    tr.process()
    assert sess.encodes == 1
    now[0] += 0.02
    _, buf = tr.process()                                  # due: the tail is encoded as source words
    assert sess.encodes == 2 and len(sess.src) == 5 and tr.last_n_accessible == 3
    assert len(buf.text.split()) == 2                      # ... and nothing is committed from it
    tr.process()                                           # unchanged tail: nothing to do
    tr.insert_tokens([Tail("gamma")])
    now[0] += 5.0
    tr.process()
    assert sess.encodes == 2
    tr.insert_tokens([Tail("gamma delta"), words("gamma", 0.8)[0]])
    tr.process()                                           # committed words run at once
    assert sess.encodes == 3
    # a session that did not ask for the tail ignores it
    _, plain = make(threshold=0, tail=False)
    plain.insert_tokens(words("alpha beta") + [Tail("gamma")])
    plain.process()
    assert len(plain.session.src) == 4


def test_n_accessible_shrinks_when_the_tokenizer_merges_across_the_boundary():
    _, tr = make(threshold=0, tail=True)
    tr.insert_tokens(words("alpha beta") + [Tail("gamma")])
    tr.process()
    assert tr.last_n_accessible == 3                       # language code + two committed words
    _, merged = make(threshold=0, tail=True, merge=("beta", "gamma"))
    merged.insert_tokens(words("alpha beta") + [Tail("gamma")])
    _, buf = merged.process()
    assert merged.last_n_accessible == 2                   # "beta" now shares a token with the tail
    assert len(buf.text.split()) == 1


def test_twelve_words_under_both_policies_over_the_standin(micro_oracle):
    """the scenario of the gpu-marked twin on the CPU: append-only text, the final from the committed prefix, fewer steps"""
    from test_translation import WordTokenizer as HashTokenizer, words as hash_words
    align_steps, local_steps, report = A.stream_twelve_words(A.AlignOracleModel(micro_oracle), HashTokenizer(), hash_words)
    print(report)
    assert 0 < align_steps < local_steps


def test_context_stop_over_the_standin(micro_oracle):
    sess = AlignOracleNllbSession(micro_oracle, 1)
    sess.model.cdims = types.SimpleNamespace(max_tgt=64)
    sess.set_alignment_heads(KAT["heads"].tolist())
    src = KAT["c3_src"]
    sess.encode(src)
    ids, al, why = nllb.alignatt_loop(sess, [2, int(KAT["c3_lang"])], len(src), len(src), 0, True, EOS, 199)
    assert why == "context" and len(ids) == 63 and len(al) == 63 and CFG.pad_token_id not in ids


def test_readout_restatement_passes_the_kernel_comparison():
    """the float32 restatement through the comparison the GPU test holds the kernel to, on the same cases"""
    import nllb_align_cases as AC
    for si in range(len(AC.SHAPES)):
        exempt = n_random = 0
        for name, kind, probs, lo, hi, limit in AC.cases_of(si):
            _report, failures, n_exempt, rows = AC.compare(kind, probs, lo, hi, limit, readout(probs, lo, hi, limit))
            assert not failures, (AC.SHAPES[si], name, failures)
            if kind == "random":
                exempt, n_random = exempt + n_exempt, n_random + rows
        assert exempt <= 0.02 * n_random


def test_diag_refuses_bad_arguments_before_touching_the_device():
    """no GPU is needed to be refused: WLK_ERR_ARG (-1), not WLK_ERR_HIP, on a machine without one"""
    import ctypes as C
    import nllb_align_cases as AC
    lib = _lib.load()
    probs = AC.random_probs(2, 2, 9, 0)
    out = np.full(64, np.nan, np.float32)
    pos = np.full(8, -7, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)           # noqa: E731
    for n, rows, S, lo, hi, limit in [(0, 2, 9, 1, 8, 0), (65, 2, 9, 1, 8, 0), (2, 0, 9, 1, 8, 0), (2, 9, 9, 1, 8, 0), (2, 2, 0, 0, 0, 0),
                                      (2, 2, 513, 1, 8, 0), (2, 2, 9, -1, 8, 0), (2, 2, 9, 1, 10, 0), (2, 2, 9, 1, 8, -1), (2, 2, 9, 1, 8, 10)]:
        assert lib.wlk_diag_nllb_align(ptr(probs), n, rows, S, lo, hi, limit, ptr(out), ptr(pos), ptr(out), ptr(out)) == -1
    assert lib.wlk_diag_nllb_align(None, 2, 2, 9, 1, 8, 0, ptr(out), ptr(pos), ptr(out), ptr(out)) == -1
    assert np.isnan(out).all() and (pos == -7).all()
