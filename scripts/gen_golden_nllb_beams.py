#!/usr/bin/env python
"""Known answers for NLLB beam search with 5 .. 8 beams from `transformers`' own `M2M100ForConditionalGeneration.generate`
(transformers 5.15.0, CPU) on the micro configuration with seeded weights - the beam widths whose 2 n continuations per row
need the wide top-k kernel.  tests/golden/nllb_kat.npz has one 5-beam and one 8-beam case that end after three
generated tokens; the cases here generate at least 12 tokens, in some of them hypotheses end before the length limit, and a length
penalty other than 1 and early_stopping=True take part.

A candidate is KEPT only if it is robust against the size of error a float32 implementation has: `nllb.beam_search` over
the CPU oracle must return the same sequence without noise, with uniform noise of +-2e-5 and with +-1e-4 (two seeds) added to
every log-probability the session hands out.  1e-4 is 5x the library's worst logit error on this shape, so "the identical
sequence on the GPU" is a fair demand of such a case.  Candidates that fail are reported and skipped.

Writes tests/golden/nllb_beam_wide_kat.npz.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED, EOS_GAIN = 1, 4.0
NOISE = ((1e-4, 11), (1e-4, 12), (2e-5, 13))          # (amplitude, seed)
# (beams, length_penalty, early_stopping, max_new_tokens, hypotheses must end before the limit).  With these weights a
# hypothesis that ends does so after 5 .. 10 tokens and, at a length penalty of 1 or less, wins: the cases in which hypotheses
# end early AND the answer has 12 tokens or more are those whose penalty favours length.
SPECS = [(5, 2.0, False, 20, True), (6, 0.6, False, 16, False), (7, 1.0, True, 18, False), (8, 1.0, False, 14, False),
         (8, 2.0, False, 16, True), (7, 1.5, False, 16, True)]
MIN_NEW = 12


def noisy_session_class():
    import torch
    from oracle.nllb_oracle import OracleNllbSession

    class NoisySession(OracleNllbSession):
        """every log-probability handed out carries uniform noise of +-amp"""

        def __init__(self, oracle, rows, amp, seed):
            super().__init__(oracle, rows)
            self.amp, self.rng = amp, np.random.default_rng(seed)

        def _lp(self):
            lp = torch.log_softmax(self.last, dim=-1).numpy()
            return (lp + self.rng.uniform(-self.amp, self.amp, lp.shape)).astype(np.float32)

        def logits(self):
            return self._lp()

        def topk(self, k):
            lp = torch.from_numpy(self._lp())
            v, i = lp.topk(k, dim=-1)
            return v.numpy(), i.numpy().astype("int32")

    return NoisySession


def main():
    import torch
    from transformers import M2M100Config, M2M100ForConditionalGeneration

    from oracle.nllb_oracle import NllbOracle, OracleNllbSession
    from whisperlivekit_amd import nllb

    cfg = nllb.NLLB_MICRO
    hf_cfg = M2M100Config(vocab_size=cfg.vocab_size, d_model=cfg.d_model, encoder_layers=cfg.encoder_layers,
                          decoder_layers=cfg.decoder_layers, encoder_attention_heads=cfg.attention_heads,
                          decoder_attention_heads=cfg.attention_heads, encoder_ffn_dim=cfg.ffn_dim, decoder_ffn_dim=cfg.ffn_dim,
                          activation_function="relu", scale_embedding=cfg.scale_embedding, pad_token_id=cfg.pad_token_id,
                          eos_token_id=cfg.eos_token_id, bos_token_id=0, decoder_start_token_id=cfg.decoder_start_token_id,
                          max_position_embeddings=cfg.max_position_embeddings, dropout=0.0, attention_dropout=0.0,
                          activation_dropout=0.0, encoder_layerdrop=0.0, decoder_layerdrop=0.0, use_cache=True)
    weights = nllb.synth_state_dict(cfg, SEED, eos_gain=EOS_GAIN)
    model = M2M100ForConditionalGeneration(hf_cfg).eval()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()}, strict=False)
    model.tie_weights()
    assert torch.equal(model.lm_head.weight, torch.from_numpy(weights["model.shared.weight"]))
    oracle = NllbOracle(cfg, weights)
    Noisy = noisy_session_class()

    rng = np.random.default_rng(20)
    out, cases = {}, []
    for beams, lp, es, max_new, want_early in SPECS:
        for attempt in range(60):
            n_src = int(rng.integers(3, 40))
            src = rng.integers(4, 1900, size=n_src).astype(np.int64)
            src[-1] = cfg.eos_token_id
            lang = 1990 + len(cases)
            def run(**kw):
                with torch.no_grad():
                    ids = model.generate(torch.from_numpy(src)[None], forced_bos_token_id=lang, num_beams=beams, do_sample=False,
                                         max_new_tokens=max_new, **kw)[0].tolist()
                return [t for t in ids if t != cfg.pad_token_id]

            seq = run(length_penalty=lp, early_stopping=es)
            n_new = len(seq) - 1
            # the running beams do not depend on the penalty, which only ranks what has ended: if the same search at penalty 1
            # answers with a hypothesis that ended early, that hypothesis sat in this search's finished slots too
            short = run(length_penalty=1.0, early_stopping=False) if want_early else seq
            early = len(short) - 1 < max_new and short[-1] == cfg.eos_token_id
            if n_new < MIN_NEW or (want_early and not early):
                continue
            kw = dict(num_beams=beams, max_new_tokens=max_new, length_penalty=lp, early_stopping=es)
            runs = [nllb.beam_search(OracleNllbSession(oracle, beams), src, lang, **kw)]
            runs += [nllb.beam_search(Noisy(oracle, beams, amp, seed), src, lang, **kw) for amp, seed in NOISE]
            if any(r != seq for r in runs):
                print(f"  {beams} beams, attempt {attempt}: not robust against the noise (or not transformers' sequence) - skipped")
                continue
            bi = len(cases)
            out[f"src{bi}"], out[f"out{bi}"] = src, np.asarray(seq, np.int64)
            cases.append((lang, beams, int(round(lp * 1000)), {False: 0, True: 1, "never": 2}[es], -1, max_new))
            print(f"case {bi}: {beams} beams, src {n_src}, length_penalty {lp}, early_stopping {es}, max_new {max_new}: "
                  f"{n_new} generated{' (hypotheses end before the limit)' if early else ''}: {seq}")
            break
        else:
            raise SystemExit(f"no robust case found for {beams} beams / {lp} / {es} / {max_new}")
    out["cases"] = np.asarray(cases, np.int64)          # columns as nllb_kat.npz's beam_cases
    out["weights"] = np.asarray([SEED, int(round(EOS_GAIN * 1000))], np.int64)
    path = os.path.join(ROOT, "tests", "golden", "nllb_beam_wide_kat.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
