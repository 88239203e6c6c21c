"""TEST INFRASTRUCTURE for the stacked AlignAtt route: CPU stand-ins for the alignment surface of
`HipNllbBatch` (set_alignment_heads / prefill / step_align / alignment / align_stats).

* `AlignOracleNllbBatch`: tests/nllb_batch_standin.py's OracleNllbBatch whose slots can also be prefilled and stepped with
  the alignment read-out - every slot is an `AlignOracleNllbSession` (tests/nllb_align_standin.py) over the slot's own
  encoder output and cache, so a row's results are that session's, whatever else shares the step.  The library's contract
  errors (csrc/nllb_batch.hip) are restated so that the host loop is tested against them too.
* `ScriptedAlignBatch` / `ScriptedAlignSession` / `ScriptedAlignModel`: a "translation" that copies, with no network, for
  the rule and the serving tests."""
import types

import numpy as np
import torch

from nllb_align_standin import AlignOracleNllbSession
from nllb_batch_standin import OracleNllbBatch


class AlignOracleNllbBatch(OracleNllbBatch):
    def __init__(self, oracle, n_slots=8, on_step=None, max_tgt=None):
        super().__init__(oracle, n_slots, on_step)
        if max_tgt is not None:
            self.model.cdims = types.SimpleNamespace(max_tgt=max_tgt)
        self.max_tgt = max_tgt
        self.heads = []
        self.sess = [None] * n_slots
        self.self_len = [0] * n_slots
        self.align_row = [None] * n_slots          # the slot's p of the latest align step
        self.n_prefills = self.n_align_steps = 0
        self.prefill_rows = []                     # rows of every prefill call
        self.align_rows = []                       # rows of every align step

    def set_alignment_heads(self, pairs):
        probe = AlignOracleNllbSession(self.oracle, 1)
        probe.set_alignment_heads(pairs)           # ValueError for a bad set
        self.heads = probe.heads
        self.align_row = [None] * self.n_slots

    def encode(self, slots, sources):
        super().encode(slots, sources)
        for s in self._check(slots):
            sess = AlignOracleNllbSession(self.oracle, 1)
            sess.enc, sess.cache = self.enc[s], self.cache[s]
            self.sess[s], self.self_len[s], self.align_row[s] = sess, 0, None

    def step(self, slots, tokens, k=1):
        out = super().step(slots, tokens, k)
        for s in slots:
            self.self_len[int(s)] += 1
        return out

    def prefill(self, slots, prompts):
        slots = self._check(slots)
        assert len(slots) == len(prompts)
        for s, pr in zip(slots, prompts):
            if self.enc[s] is None or self.self_len[s] != 0:
                raise RuntimeError("prefill on a slot that is not encoded or already holds target tokens")
            if len(pr) < 1:
                raise ValueError("every prompt needs at least one token")
            if self.max_tgt is not None and len(pr) > self.max_tgt - 1:
                raise OverflowError("a prompt leaves no room for a step")
        for s, pr in zip(slots, prompts):
            self.oracle.decode(torch.tensor([[int(t) for t in pr]]), self.enc[s], self.cache[s])
            self.self_len[s] = len(pr)
        self.n_prefills += 1
        self.prefill_rows.append(sum(len(pr) for pr in prompts))

    def step_align(self, slots, tokens, k, lo, hi, limit):
        slots = self._check(slots)
        assert len(slots) == len(tokens) == len(lo) == len(hi) == len(limit)
        if not self.heads:
            raise RuntimeError("step_align before set_alignment_heads")
        for s, l, h, m in zip(slots, lo, hi, limit):
            if self.enc[s] is None or self.self_len[s] == 0:
                raise RuntimeError("step_align on a slot without a prompt")
            S = self.enc[s].shape[-2]
            if l < 0 or h > S or m < 0 or m > S:
                raise ValueError("needs 0 <= lo, hi <= src_len and 0 <= limit <= src_len")
            if self.max_tgt is not None and self.self_len[s] + 1 > self.max_tgt:
                raise OverflowError("target context exceeded")
        if self.on_step is not None:
            self.on_step(self, slots)
        n = len(slots)
        lp, ids = np.empty((n, k), np.float32), np.empty((n, k), np.int32)
        pos, prob, mass = np.empty(n, np.int32), np.empty(n, np.float32), np.empty(n, np.float32)
        self.align_row = [None] * self.n_slots
        for r, s in enumerate(slots):
            sess = self.sess[s]
            sess.heads = self.heads
            lp[r], ids[r], pos[r:r + 1], prob[r:r + 1], mass[r:r + 1] = sess.step_align([int(tokens[r])], k, int(lo[r]), int(hi[r]),
                                                                                     int(limit[r]))
            self.last[s] = sess.last[0]
            self.align_row[s] = sess.alignment()[0]
            self.self_len[s] += 1
        self.n_steps += 1
        self.n_rows += n
        self.n_align_steps += 1
        self.align_rows.append(n)
        return lp, ids, pos, prob, mass

    def release(self, slot):
        super().release(slot)
        self.sess[slot], self.self_len[slot], self.align_row[slot] = None, 0, None

    def alignment(self, slot):
        if self.align_row[slot] is None:
            raise RuntimeError("the slot was not in the latest align step")
        return self.align_row[slot].copy()

    def align_stats(self):
        return {"align_steps": self.n_align_steps, "graph_captures": 0}


# ---- the copying "translation" --------------------------------------------------------------------------------------------
END_MARKER = 777       # a source content id whose target token is </s>: the sentence "ends early" at that position


def scripted_token(cfg, src, t, lookahead, lo, hi):
    """target token t (behind [</s>, language]) of the copy: content id + 1000 leaning on source position 1 + t (+ lookahead);
    </s> behind the content or at END_MARKER, leaning on the position it stands for"""
    content = src[1:-1]
    y = cfg.eos_token_id if t >= len(content) or content[t] == END_MARKER else content[t] + 1000
    a = min(1 + t + lookahead, len(src) - 2)
    return y, (a if lo <= a < hi else -1)


class ScriptedAlignSession:
    """what generate_alignatt (device_loop=False) calls on a 1-row session, answered by the copy"""

    def __init__(self, cfg, lookahead=0):
        self.rows, self.model, self.lookahead = 1, types.SimpleNamespace(cfg=cfg), lookahead
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
        y, a = scripted_token(self.model.cfg, self.src, len(self.fed) - 2, self.lookahead, lo, hi)
        return np.zeros((1, 1), np.float32), np.asarray([[y]], np.int32), np.asarray([a], np.int32), None, None

    def close(self):
        pass


class ScriptedAlignBatch:
    """the same copy per slot, with the library's slot rules; counts what the host loop asks for"""

    def __init__(self, cfg, n_slots=8, lookahead=0, on_step=None, max_tgt=None):
        self.n_slots, self.lookahead, self.on_step, self.max_tgt = n_slots, lookahead, on_step, max_tgt
        self.model = types.SimpleNamespace(cfg=cfg)
        if max_tgt is not None:
            self.model.cdims = types.SimpleNamespace(max_tgt=max_tgt)
        self.src, self.fed = [None] * n_slots, [None] * n_slots
        self.heads, self.closed = None, False
        self.encodes, self.prefills, self.steps = [], [], []       # slots of every encode / prompt lengths / slots of every step
        self.released = []

    def _check(self, slots):
        slots = [int(s) for s in slots]
        if not slots or len(set(slots)) != len(slots) or any(s < 0 or s >= self.n_slots for s in slots):
            raise ValueError("bad slots")
        return slots

    def set_alignment_heads(self, pairs):
        self.heads = list(pairs)

    def encode(self, slots, sources):
        slots = self._check(slots)
        assert len(slots) == len(sources)
        for s, src in zip(slots, sources):
            assert self.src[s] is None, "encode into a slot that was not released"
            self.src[s], self.fed[s] = [int(v) for v in src], []
        self.encodes.append(slots)

    def prefill(self, slots, prompts):
        slots = self._check(slots)
        assert len(slots) == len(prompts)
        for s, pr in zip(slots, prompts):
            if self.src[s] is None or self.fed[s]:
                raise RuntimeError("prefill on a slot that is not fresh")
            if len(pr) < 1 or (self.max_tgt is not None and len(pr) > self.max_tgt - 1):
                raise ValueError("bad prompt length")
            self.fed[s] = [int(t) for t in pr]
        self.prefills.append([len(pr) for pr in prompts])

    def step_align(self, slots, tokens, k, lo, hi, limit):
        slots = self._check(slots)
        assert self.heads, "step_align before set_alignment_heads"
        assert len(slots) == len(tokens) == len(lo) == len(hi) == len(limit) and k == 1
        if self.on_step is not None:
            self.on_step(self, slots)
        ids, pos = np.empty((len(slots), 1), np.int32), np.empty(len(slots), np.int32)
        for r, s in enumerate(slots):
            if self.src[s] is None or not self.fed[s]:
                raise RuntimeError("step_align on a slot without a prompt")
            if self.max_tgt is not None and len(self.fed[s]) + 1 > self.max_tgt:
                raise OverflowError("target context exceeded")
            assert 0 <= lo[r] and hi[r] <= len(self.src[s]) and 0 <= limit[r] <= len(self.src[s])
            self.fed[s].append(int(tokens[r]))
            ids[r, 0], pos[r] = scripted_token(self.model.cfg, self.src[s], len(self.fed[s]) - 2, self.lookahead, lo[r], hi[r])
        self.steps.append(slots)
        return np.zeros((len(slots), 1), np.float32), ids, pos, None, None

    def release(self, slot):
        self._check([slot])
        self.src[slot] = self.fed[slot] = None
        self.released.append(int(slot))

    def close(self):
        self.closed = True


class ScriptedAlignModel:
    """what HipNllbTranslationModel needs from a HipNllbModel"""

    def __init__(self, cfg, lookahead=0, on_step=None):
        self.cfg, self.lookahead, self.on_step = cfg, lookahead, on_step
        self.sessions, self.batches = [], []

    def new_session(self, rows=1):
        self.sessions.append(ScriptedAlignSession(self.cfg, self.lookahead))
        return self.sessions[-1]

    def new_batch(self, n_slots=8):
        self.batches.append(ScriptedAlignBatch(self.cfg, n_slots, self.lookahead, self.on_step))
        return self.batches[-1]


class HashTokenizer:
    """one id per word: [language code] words </s> (the `transformers` tokenizer surface translation.py uses)"""
    unk_token_id = 3
    LANGS = {"eng_Latn": 1990, "fra_Latn": 1991, "deu_Latn": 1992}

    def __init__(self, eos):
        self.src_lang, self.eos = "eng_Latn", eos

    @staticmethod
    def word_id(w):
        h = 0
        for ch in w:
            h = (h * 131 + ord(ch)) % 700
        return 10 + h                                  # below END_MARKER

    def __call__(self, text):
        return types.SimpleNamespace(input_ids=[self.LANGS[self.src_lang]] + [self.word_id(w) for w in text.lower().split()] + [self.eos])

    def convert_tokens_to_ids(self, tok):
        return self.LANGS.get(tok, self.unk_token_id)

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(f"w{int(i)}" for i in ids)


def all_requests(kat, settings_of):
    """every stored setting of every micro case of tests/golden/nllb_align_kat.npz as one request list
    -> ([request], [wanted outcome])"""
    reqs, want = [], []
    for ci in range(int(kat["n_cases"])):
        prefix = f"c{ci}_"
        for _k, n_acc, thr, final, committed, max_new, ids, align, why in settings_of(kat, prefix):
            reqs.append((kat[prefix + "src"].tolist(), int(kat[prefix + "lang"]), committed, n_acc, thr, final, max_new))
            want.append((ids, align, why))
    return reqs, want
