#!/usr/bin/env python
"""Known answers for the stacked NLLB path (whisperlivekit_amd.nllb.HipNllbBatch / generate_batch, csrc/nllb_batch.hip)
from `transformers`' own M2M100ForConditionalGeneration (5.15.0), in the manner of gen_golden_nllb.py: the micro
configuration with the seeded weights of whisperlivekit_amd.nllb.synth_state_dict, and for each of 12 source sentences of
ragged length - every one with its own target language id and its own max_new_tokens - what the network gives for that
sentence ALONE:

* the encoder output,
* `model.generate(num_beams=1, do_sample=False, forced_bos_token_id=lang, max_new_tokens=n)`,
* the logits of the first 4 decoder steps, teacher-forced along that output (padded with fixed ids where it is shorter).

A stacked pass must reproduce each of them, whatever else shares its launches.  At least 3 sentences have to end by
`</s>` before their limit and at least 3 have to run into it (refill in the middle of a decode needs both); with
eos_gain 6 only one of twelve random sources ended early, so the `</s>` gain is raised until the mix is there, and the
mix is asserted here and again by the test.

Writes tests/golden/nllb_batch_kat.npz.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (source length, target language id, max_new_tokens): 1, a few below 10, two of equal length, one >= 64, one at
# 90 = max_src - 2 of the test model
SPECS = [(1, 1990, 8), (3, 1991, 4), (5, 1992, 24), (7, 1993, 40), (9, 1994, 12), (9, 1995, 30), (17, 1996, 6), (30, 1997, 36),
         (64, 1998, 20), (90, 1999, 16), (12, 1990, 40), (20, 1993, 28)]
SEED = 0
N_LOGIT_STEPS = 4


def build(cfg, eos_gain):
    import torch
    from transformers import M2M100Config, M2M100ForConditionalGeneration

    from whisperlivekit_amd import nllb
    hf_cfg = M2M100Config(vocab_size=cfg.vocab_size, d_model=cfg.d_model, encoder_layers=cfg.encoder_layers,
                          decoder_layers=cfg.decoder_layers, encoder_attention_heads=cfg.attention_heads,
                          decoder_attention_heads=cfg.attention_heads, encoder_ffn_dim=cfg.ffn_dim, decoder_ffn_dim=cfg.ffn_dim,
                          activation_function="relu", scale_embedding=cfg.scale_embedding, pad_token_id=cfg.pad_token_id,
                          eos_token_id=cfg.eos_token_id, bos_token_id=0, decoder_start_token_id=cfg.decoder_start_token_id,
                          max_position_embeddings=cfg.max_position_embeddings, dropout=0.0, attention_dropout=0.0,
                          activation_dropout=0.0, encoder_layerdrop=0.0, decoder_layerdrop=0.0, use_cache=True)
    model = M2M100ForConditionalGeneration(hf_cfg).eval()
    sd = {k: torch.from_numpy(v) for k, v in nllb.synth_state_dict(cfg, SEED, eos_gain).items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    tied = {"lm_head.weight", "model.encoder.embed_tokens.weight", "model.decoder.embed_tokens.weight"}
    assert set(missing) <= tied and not unexpected, (missing, unexpected)
    model.tie_weights()
    assert torch.equal(model.lm_head.weight, sd["model.shared.weight"])
    return model


def main():
    import torch

    from whisperlivekit_amd import nllb

    cfg = nllb.NLLB_MICRO
    rng = np.random.default_rng(11)
    sources = []
    for n_src, _lang, _max_new in SPECS:
        src = rng.integers(4, 1900, size=n_src).astype(np.int64)
        src[-1] = cfg.eos_token_id                                   # NLLB sources end with </s> (and contain it only there)
        sources.append(src)
    chosen = None
    for eos_gain in (6.0, 8.0, 10.0, 12.0, 14.0, 16.0, 20.0, 24.0):
        model = build(cfg, eos_gain)
        gens = []
        with torch.no_grad():
            for src, (_n, lang, max_new) in zip(sources, SPECS):
                gens.append(model.generate(torch.from_numpy(src)[None], forced_bos_token_id=lang, num_beams=1, do_sample=False,
                                           max_new_tokens=max_new)[0].numpy().astype(np.int64))
        early = sum(1 for g, (_n, _l, mn) in zip(gens, SPECS) if int(g[-1]) == cfg.eos_token_id and len(g) < 1 + mn)
        at_limit = sum(1 for g, (_n, _l, mn) in zip(gens, SPECS) if len(g) == 1 + mn and int(g[-1]) != cfg.eos_token_id)
        print(f"eos_gain {eos_gain}: {early} end by </s> before their limit, {at_limit} run into it")
        if early >= 3 and at_limit >= 3:
            chosen = (eos_gain, model, gens)
            break
    assert chosen is not None, "no eos_gain gave 3 early endings and 3 sentences at their limit"
    eos_gain, model, gens = chosen
    out = {"seed": np.int64(SEED), "eos_gain": np.float64(eos_gain), "cases": np.asarray(SPECS, np.int64)}
    for i, (src, gen, (_n, lang, _mn)) in enumerate(zip(sources, gens, SPECS)):
        forced = list(gen[:N_LOGIT_STEPS]) + [10 + i, 20 + i, 30 + i][: max(0, N_LOGIT_STEPS - len(gen))]
        forced = np.asarray(forced, np.int64)
        with torch.no_grad():
            ids = torch.from_numpy(src)[None]
            enc = model.model.encoder(input_ids=ids).last_hidden_state[0]
            logits = model(input_ids=ids, decoder_input_ids=torch.from_numpy(forced)[None]).logits[0]
        out[f"src{i}"], out[f"gen{i}"], out[f"fed{i}"] = src, gen, forced
        out[f"enc{i}"] = enc.numpy().astype(np.float32)
        out[f"logits{i}"] = logits.numpy().astype(np.float32)
        print(f"sentence {i}: {len(src)} source ids, language {lang}, limit {_mn}: {len(gen)} ids, ends {int(gen[-1])}")
    path = os.path.join(ROOT, "tests", "golden", "nllb_batch_kat.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size < 1024 * 1024, "the fixture must stay under the size limit for committed files"


if __name__ == "__main__":
    main()
