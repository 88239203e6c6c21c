"""TEST INFRASTRUCTURE for NLLB draft verification: the fixture tests/golden/nllb_draft_kat.npz
(scripts/gen_golden_nllb_draft.py), the float64 form of the repository's CPU oracle that produced it, and the stand-in batch
of the CPU tests.

A token comparison is only meaningful where no kernel within tolerance can flip the pick, so every truth of the fixture
carries, per generated token, the float64 gap between the best and the second-best logit, and every truth used keeps
gap >= GAP_MIN = 2e-3 = twice tests/test_nllb.py's LOGIT_ATOL (600M shape: BIG_GAP_MIN = 1e-2 = twice the 5e-3 of
test_hip_600m_shape_matches_the_oracle).  A candidate that misses the gap is replaced when the fixture is generated."""
import numpy as np
import torch

import helpers as H
from nllb_batch_standin import OracleNllbBatch
from oracle.nllb_oracle import NllbOracle
from whisperlivekit_amd import nllb

GAP_MIN = 2e-3
BIG_GAP_MIN = 1e-2
MAX_TGT = 80          # the target context of the GPU tests' micro model
CFG = nllb.NLLB_MICRO
BIG_CFG = nllb.NLLB_200_DISTILLED_600M
BIG_MAX_SRC, BIG_MAX_TGT = 64, 32


def float64_oracle(cfg, sd) -> NllbOracle:
    """oracle/nllb_oracle.py with every parameter, the position table and the activations in float64 (the fp32 parameter
    values, exactly)."""
    o = NllbOracle(cfg, sd)
    o.sd = {k: v.double() for k, v in o.sd.items()}
    o.emb = o.sd["model.shared.weight"]
    o.pos = o.pos.double()
    return o


def _gap(row: torch.Tensor):
    top = row.topk(2)
    return int(top.indices[0]), float(top.values[0] - top.values[1])


def greedy_with_gaps(o64: NllbOracle, src, lang: int, max_new: int):
    """nllb.generate's rule (forced first token, </s> or the length stop) on the float64 oracle -> (ids, gaps): gaps[j] is
    the best-minus-second logit where ids[2 + j] was picked."""
    cfg = o64.cfg
    enc, cache = o64.encode([int(t) for t in src]), o64.new_cache()
    out, gaps = [cfg.decoder_start_token_id], []
    for _ in range(max_new):
        row = o64.decode(torch.tensor([[out[-1]]]), enc, cache)[0, -1]
        if len(out) == 1:
            out.append(int(lang))
            continue
        best, gap = _gap(row)
        out.append(best)
        gaps.append(gap)
        if best == cfg.eos_token_id:
            break
    return out, np.asarray(gaps, np.float64)


def forced_gaps(o64: NllbOracle, src, ids):
    """One teacher-forced pass over ids[:-1] -> (picks, gaps) at the positions of ids[2:]: a truth is greedy iff picks == ids[2:]."""
    enc = o64.encode([int(t) for t in src])
    rows = o64.decode(torch.tensor([[int(t) for t in ids[:-1]]]), enc, o64.new_cache())[0, 1:]
    got = [_gap(r) for r in rows]
    return [g[0] for g in got], np.asarray([g[1] for g in got], np.float64)


class Fixture:
    def __init__(self):
        z = H.golden_npz("nllb_draft_kat.npz")
        self.z = z
        self.weights = dict(seed=int(z["seed"]), eos_gain=float(z["eos_gain"]))
        self.cases = [tuple(int(v) for v in row) for row in z["cases"]]          # (language id, max_new_tokens)
        self.n = len(self.cases)
        self.src = [z[f"src{i}"].astype(np.int64) for i in range(self.n)]
        self.gen = [z[f"gen{i}"].tolist() for i in range(self.n)]
        self.gap = [z[f"gap{i}"] for i in range(self.n)]
        self.lang = [c[0] for c in self.cases]
        self.limit = [c[1] for c in self.cases]
        self.big = dict(seed=int(z["big_seed"]), src=z["big_src"].astype(np.int64), lang=int(z["big_lang"]),
                        limit=int(z["big_max_new"]), gen=z["big_gen"].tolist(), gap=z["big_gap"])

    def micro_weights(self):
        return nllb.synth_state_dict(CFG, self.weights["seed"], self.weights["eos_gain"])

    def ends_by_eos(self, i):
        return self.gen[i][-1] == CFG.eos_token_id and len(self.gen[i]) < 1 + self.limit[i]

    def long_case(self):
        return next(i for i in range(self.n) if len(self.gen[i]) >= 70)


class VerifyingOracleNllbBatch(OracleNllbBatch):
    """OracleNllbBatch plus `verify` by ONE teacher-forced oracle decode per slot: the contract of wlk_nllb_batch_verify
    restated on the CPU (state rules, picks, the accepted prefix, the cache cut back to 2 + k positions)."""

    def __init__(self, oracle, n_slots=8, on_step=None, max_tgt=MAX_TGT):
        super().__init__(oracle, n_slots, on_step)
        self.model.cdims = type("Dims", (), {"max_tgt": max_tgt})()
        self.max_tgt = max_tgt
        self.n_verifies = self.n_verify_rows = self.n_draft = self.n_accepted = 0
        self.verify_calls = []                   # per call: [(slot, accepted, draft length)]

    def verify(self, slots, token_lists):
        slots = self._check(slots)
        assert len(slots) == len(token_lists)
        accepted, nxt, call = [], [], []
        for s, toks in zip(slots, token_lists):
            toks = [int(t) for t in toks]
            if self.enc[s] is None:
                raise RuntimeError("verify on a slot that is not encoded")
            if self.cache[s]["k"][0] is not None:
                raise RuntimeError("verify on a slot that already holds target tokens")
            if len(toks) < 2 or len(toks) > self.max_tgt - 1:
                raise ValueError("verify: 2 .. max_tgt - 1 tokens per slot")
            cfg = self.oracle.cfg
            if any(t < 0 or t >= cfg.vocab_size or t == cfg.pad_token_id for t in toks):
                raise ValueError("token id out of range")
            rows = self.oracle.decode(torch.tensor([toks]), self.enc[s], self.cache[s])[0]
            picks = [int(r.argmax()) for r in rows[1:]]
            d = toks[2:]
            k = next((j for j in range(len(d)) if picks[j] != d[j]), len(d))
            for i in range(len(self.cache[s]["k"])):                      # the slot holds 2 + k positions afterwards
                self.cache[s]["k"][i] = self.cache[s]["k"][i][:, :2 + k]
                self.cache[s]["v"][i] = self.cache[s]["v"][i][:, :2 + k]
            self.last[s] = None
            accepted.append(k)
            nxt.append(picks[k])
            call.append((s, k, len(d)))
            self.n_verify_rows += len(toks)
            self.n_draft += len(d)
            self.n_accepted += k
        self.n_verifies += 1
        self.verify_calls.append(call)
        return np.asarray(accepted, np.int32), np.asarray(nxt, np.int64)

    def verify_stats(self):
        return {"passes": self.n_verifies, "draft_tokens": self.n_draft, "accepted_tokens": self.n_accepted}


# ---- growing sentences for the serving tests --------------------------------------------------------------------------------
WORDS = "the quick brown fox jumps over lazy dog and then it sleeps hello again friend new sentence here last words".split()
SCREENED_LIMIT = 8            # max_new_tokens of the screened serving runs


def growing_script(seed, n_words=8, reset_at=None):
    """One word per update, the last one closes the sentence: [("tokens", [ASRToken])] * n_words; reset_at: a silence start
    (validate_buffer_and_reset) behind that many words."""
    from test_translation import words
    rng = np.random.default_rng(seed)
    picked = [WORDS[int(k)] for k in rng.integers(0, len(WORDS), size=n_words)]
    picked[-1] += "."
    script = [("tokens", words(w, 0.4 * j)) for j, w in enumerate(picked)]
    if reset_at is not None:
        script.insert(reset_at, ("reset", None))
    return script


def drive_script(tm, script, target="fra_Latn"):
    """The calls of translation_processor for a scripted session -> (log of (kind, new piece, buffer), session)."""
    tr = tm.new_session("eng_Latn", target)
    log = []
    for kind, arg in script:
        if kind == "tokens":
            tr.insert_tokens(arg)
            new, buf = tr.process()
        else:
            new, buf = tr.validate_buffer_and_reset()
        log.append((kind, None if new is None else (new.start, new.end, new.text), (buf.start, buf.end, buf.text)))
    return log, tr


class GapRecordingBatch(OracleNllbBatch):
    """OracleNllbBatch that keeps the best-minus-second logit of every pick a pass makes (a slot's first step predicts the
    forced language token and is no pick)."""

    def __init__(self, oracle, n_slots=8):
        super().__init__(oracle, n_slots)
        self.gaps = []

    def step(self, slots, tokens, k=1):
        slots = self._check(slots)
        picks = [self.cache[s]["k"][0] is not None for s in slots]
        out = super().step(slots, tokens, k)
        self.gaps += [_gap(self.last[s])[1] for s, is_pick in zip(slots, picks) if is_pick]
        return out


# seeds of growing_script whose every hypothesis (SCREENED_LIMIT tokens at most, either target language) keeps gap >= GAP_MIN
# on the float64 oracle: found by scanning, asserted by tests/test_nllb_draft_cpu.py
SCREENED_SEEDS = (8, 10, 12, 14)
SCREENED_TARGETS = ("fra_Latn", "deu_Latn")
RESET_SCRIPT = dict(seed=10, n_words=10, reset_at=4)     # the same condition, target fra_Latn, with a silence start inside
