#!/usr/bin/env python
"""Known answers for AlignAtt streaming translation from `transformers`' own
M2M100ForConditionalGeneration (5.15.0 in this image) with attn_implementation="eager", which returns the decoder's
cross-attention probabilities.

Weights: whisperlivekit_amd.nllb.synth_state_dict(NLLB_MICRO, 0) with `encoder_attn.q_proj` weight and bias of every decoder
layer multiplied by GAIN = 8.  Seeded weights attend almost flatly - the two largest head-mean probabilities of a row lie
about 1e-5 apart, and an arg-max over such a row pins nothing; at gain 8 they lie 2e-3 or more apart and the arg-max moves between
steps.  (`tests/nllb_align_standin.py: align_gain_state_dict` builds these weights, here and in the tests.)

Per case (sources [language, content..., </s>] of 3, 5, 17, 33, 64 and 90 ids, 12 greedy steps each, heads = every head of
decoder layer 1):
* the source, the target language and the greedy candidates y_t (step t feeds [lang, y_0, y_1, ...][t]);
* per step p = mean over the heads of their cross-attention row, from a float64 copy of the model (`p64`) and from the
  float32 model (`p32`); the arg-max of p64 over the content window [1, S - 1) (`pos`) and the gap between the two largest
  values of that window (`gap`; inf for a window of one);
* the outcome (ids, alignments, stop reason) of the rule of DESIGN 21 for several (n_accessible, threshold, final,
  committed prefix length, max_new) settings, restated here over the stored float64 steps.
Asserted here, so that no test needs an exemption: every stored gap exceeds 4e-4; float32 and float64 pick the same tokens
and positions; among the non-final outcomes there is a stop at step 0, a stop after 3 or more tokens, and a run that ends
on its length.

One more case at the NLLB-200-distilled-600M dimensions (seed 1 and the source of scripts/gen_golden_nllb_600m.py, 23 ids,
4 greedy steps, every head of decoder layer 6, the same gain), prefixed `big_`.

Writes tests/golden/nllb_align_kat.npz.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from nllb_align_standin import GAIN, align_gain_state_dict  # noqa: E402  (the tests rebuild the same weights with it)

GOLDEN = os.path.join(ROOT, "tests", "golden", "nllb_align_kat.npz")
N_STEPS = 12
REASONS = ("attention", "eos", "length", "context")


def build_model(cfg, sd):
    import torch
    from transformers import M2M100Config, M2M100ForConditionalGeneration
    hf_cfg = M2M100Config(vocab_size=cfg.vocab_size, d_model=cfg.d_model, encoder_layers=cfg.encoder_layers,
                          decoder_layers=cfg.decoder_layers, encoder_attention_heads=cfg.attention_heads,
                          decoder_attention_heads=cfg.attention_heads, encoder_ffn_dim=cfg.ffn_dim, decoder_ffn_dim=cfg.ffn_dim,
                          activation_function="relu", scale_embedding=cfg.scale_embedding, pad_token_id=cfg.pad_token_id,
                          eos_token_id=cfg.eos_token_id, bos_token_id=0, decoder_start_token_id=cfg.decoder_start_token_id,
                          max_position_embeddings=cfg.max_position_embeddings, dropout=0.0, attention_dropout=0.0,
                          activation_dropout=0.0, encoder_layerdrop=0.0, decoder_layerdrop=0.0, use_cache=True,
                          attn_implementation="eager")
    model = M2M100ForConditionalGeneration(hf_cfg).eval()
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    tied = {"lm_head.weight", "model.encoder.embed_tokens.weight", "model.decoder.embed_tokens.weight"}
    assert set(missing) <= tied and not unexpected, (missing, unexpected)
    model.tie_weights()
    return model


def forward(model, src, dec, layer):
    """-> (logits [n, V], head-mean cross-attention of `layer` [n, S]) for decoder inputs `dec`, as float64 numpy"""
    import torch
    with torch.no_grad():
        r = model(input_ids=torch.from_numpy(src)[None], decoder_input_ids=torch.tensor([dec]), output_attentions=True,
                  use_cache=False)
    att = r.cross_attentions[layer][0]                     # [H, n, S]
    return r.logits[0].double().numpy(), att.double().mean(dim=0).numpy()


def greedy_steps(model, src, lang, cfg, n_steps, layer):
    """step t feeds [lang, y_0, ...][t] behind [</s>] and yields y_t; stops after the step that yields </s>"""
    dec = [cfg.decoder_start_token_id, lang]
    ys = []
    for _ in range(n_steps):
        logits, _ = forward(model, src, dec, layer)
        ys.append(int(logits[-1].argmax()))
        if ys[-1] == cfg.eos_token_id:
            break
        dec.append(ys[-1])
    return ys


def window_argmax(p, lo, hi):
    """-> (first arg-max of p[lo:hi] or -1, gap between the two largest values there)"""
    if hi <= lo:
        return -1, np.inf
    w = p[lo:hi]
    a = int(np.argmax(w))
    gap = np.inf if len(w) == 1 else float(w[a] - np.delete(w, a).max())
    return lo + a, gap


def rule(ys, pos, S, eos, n_accessible, threshold, final, committed, max_new):
    """the rule of DESIGN 21 over stored steps: step t = len(committed prefix) + tokens emitted so far"""
    lo = 1
    limit = min(max(n_accessible - threshold, lo), S)
    out, al = [], []
    while True:
        if len(out) >= max_new:
            return out, al, "length"
        t = committed + len(out)
        y, a = ys[t], pos[t]
        if not final and (a < 0 or a >= limit):
            return out, al, "attention"
        if y == eos:
            return out, al, "eos"
        out.append(y)
        al.append(a)


def one_case(prefix, out, cfg, m32, m64, src, lang, n_steps, layer, settings_of):
    S = len(src)
    ys = greedy_steps(m32, src, lang, cfg, n_steps, layer)
    dec = [cfg.decoder_start_token_id, lang] + ys[:-1]
    lg64, p64 = forward(m64, src, dec, layer)
    lg32, p32 = forward(m32, src, dec, layer)
    p64, p32 = p64[1:], p32[1:]                            # row t + 1 of the forward = step t
    assert [int(r.argmax()) for r in lg64[1:]] == ys, "float64 and float32 pick different tokens"
    pos, gaps = zip(*(window_argmax(r, 1, S - 1) for r in p64))
    pos32 = [window_argmax(r, 1, S - 1)[0] for r in p32]
    assert list(pos) == pos32, "float64 and float32 pick different positions"
    err32 = float(np.abs(p32 - p64).max())
    out[prefix + "src"], out[prefix + "lang"] = src, np.int64(lang)
    out[prefix + "greedy"] = np.asarray(ys, np.int64)
    out[prefix + "p64"], out[prefix + "p32"] = p64.astype(np.float64), p32.astype(np.float32)
    out[prefix + "pos"], out[prefix + "gap"] = np.asarray(pos, np.int64), np.asarray(gaps, np.float64)
    settings = settings_of(S, ys)
    outcomes = []
    for k, (n_acc, thr, final, c, max_new) in enumerate(settings):
        ids, al, why = rule(ys, pos, S, cfg.eos_token_id, n_acc, thr, bool(final), c, max_new)
        out[f"{prefix}out_ids{k}"], out[f"{prefix}out_align{k}"] = np.asarray(ids, np.int64), np.asarray(al, np.int64)
        outcomes.append((final, len(ids), why))
    out[prefix + "settings"] = np.asarray(settings, np.int64).reshape(-1, 5)
    out[prefix + "reasons"] = np.asarray([REASONS.index(o[2]) for o in outcomes], np.int64)
    finite = [g for g in gaps if np.isfinite(g)]
    print(f"{prefix or 'case'} S {S}: y {ys}, pos {list(pos)}, smallest gap {min(finite) if finite else float('inf'):.3e}, "
          f"float32 error {err32:.2e}, outcomes {[(o[1], o[2]) for o in outcomes]}")
    return min(finite) if finite else np.inf, err32, outcomes


def micro_settings(S, ys):
    """(n_accessible, threshold, final, committed prefix length, max_new); committed prefixes hold no </s>"""
    n = len(ys)
    c3 = min(3, n - 1)
    full = [(S, 0, 0, 0, n), (S, 2, 0, 0, n), (S - 1, 0, 0, 0, n), (max(S // 2 + 1, 1), 0, 0, 0, n),
            (max(S // 2 + 1, 1), 2, 0, c3, n - c3), (min(2, S), 0, 0, 0, n), (S, 0, 0, c3, n - c3), (S, 0, 0, 0, min(4, n)),
            (S - 1, 2, 1, 0, n), (S // 2, 2, 1, c3, n - c3), (S, 0, 1, 0, min(4, n)), (0, 0, 0, 0, n), (S, 0, 0, 0, 0)]
    return full


def main():
    import torch

    from whisperlivekit_amd import nllb

    torch.set_num_threads(8)
    out = {}
    cfg = nllb.NLLB_MICRO
    layer = cfg.decoder_layers // 2
    sd = align_gain_state_dict(cfg, 0)
    m32 = build_model(cfg, sd)
    m64 = build_model(cfg, sd).double()
    rng = np.random.default_rng(11)
    worst_gap, worst_err, all_outcomes = np.inf, 0.0, []
    sizes = (3, 5, 17, 33, 64, 90)
    for ci, S in enumerate(sizes):
        src = np.concatenate([[1980 + ci], rng.integers(4, 1900, size=S - 2), [cfg.eos_token_id]]).astype(np.int64)
        gap, err, outcomes = one_case(f"c{ci}_", out, cfg, m32, m64, src, 1990 + ci, N_STEPS, layer, micro_settings)
        worst_gap, worst_err = min(worst_gap, gap), max(worst_err, err)
        all_outcomes += outcomes
    assert worst_gap > 4e-4, worst_gap
    open_runs = [(n, why) for final, n, why in all_outcomes if not final]
    assert any(n == 0 and why == "attention" for n, why in open_runs), "no stop at step 0"
    assert any(n >= 3 and why == "attention" for n, why in open_runs), "no stop at step 3 or later"
    assert any(why == "length" and n > 0 for n, why in open_runs), "no run that ends on its length"
    out["n_cases"] = np.int64(len(sizes))
    out["gain"], out["heads"] = np.float64(GAIN), np.asarray([(layer, h) for h in range(cfg.attention_heads)], np.int64)
    print(f"micro: smallest gap {worst_gap:.3e}, largest float32 error {worst_err:.2e}")

    # ---- the 600M dimensions
    from gen_golden_nllb_600m import SEED, source_ids
    big = nllb.NLLB_200_DISTILLED_600M
    sd = align_gain_state_dict(big, SEED)
    b32 = build_model(big, sd)
    b64 = build_model(big, sd).double()
    del sd
    gap, err, _ = one_case("big_", out, big, b32, b64, source_ids(), 256057, 4, big.decoder_layers // 2,
                           lambda S, ys: [(S, 0, 0, 0, len(ys)), (S // 2, 0, 0, 0, len(ys)), (S, 0, 1, 0, len(ys))])
    out["big_seed"] = np.int64(SEED)
    out["big_heads"] = np.asarray([(big.decoder_layers // 2, h) for h in range(big.attention_heads)], np.int64)
    print(f"600M shape: smallest gap {gap:.3e}, float32 error {err:.2e}")
    np.savez_compressed(GOLDEN, **out)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
