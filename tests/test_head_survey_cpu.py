"""The alignment-head survey without a GPU: the references of tests/head_survey_reference.py against torch in float64, the
conditions the case generator (tests/head_survey_cases.py) promises the GPU test, the host half of
whisperlivekit_amd/alignment_heads.py (fold_clip against the reference script's torch expressions, the mask dump, the
custom_alignment_heads resolver) and the planted-head fixture on the CPU oracle."""
import json
import os

import numpy as np
import pytest
import torch

import head_survey_cases as HC
import head_survey_reference as HR
from whisperlivekit_amd import alignment_heads as AH
from whisperlivekit_amd.dims import ALIGNMENT_HEADS, MODEL_DIMS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("name", HC.NAMES)
def test_reference_is_the_softmax_peak_and_the_case_keeps_its_promises(name):
    c, ref = HC.case(name), HC.reference(name)
    L, H, P, F, Tk = c["n_layer"], c["n_head"], c["P"], c["F"], c["Tk"]
    assert c["ldkv"] == L * 2 * 64 * H and c["q"].shape == (L, P, 64 * H) and c["k"].shape == (Tk, c["ldkv"])
    k = c["k"].reshape(Tk, L, 2, H, 64)
    assert np.isfinite(c["q"]).all() and np.isfinite(k[:F, :, 0]).all()
    assert np.isnan(k[F:]).all() and np.isnan(k[:, :, 1]).all()          # keys at or beyond F, and every V half
    # the float64 statement is softmax(...).max() and the first arg-max
    s = torch.from_numpy(HR.scores(c))
    w = s.softmax(-1)
    assert np.allclose(ref["peak64"], w.max(-1).values.numpy(), rtol=1e-12, atol=0)
    assert np.allclose(ref["denom64"] * ref["peak64"], 1.0, rtol=1e-14)
    assert (ref["denom64"] >= 1).all()
    top = s.max(-1, keepdim=True).values
    first = torch.where(s == top, torch.arange(F).expand_as(s), F).min(-1).values.numpy()
    assert np.array_equal(ref["frame64"], first)
    # the float32 restatement is float32 throughout and close
    assert ref["denom32"].dtype == np.float32
    assert np.abs(ref["denom32"] / ref["denom64"] - 1).max() < 1e-3
    # scores within 100; the lead of the top score over every distinct runner-up
    assert ref["smax"] <= 100
    gap = ref["gap"].copy()
    gap[:, :, list(c["equal_rows"])] = np.inf
    assert (gap >= HC.GAP).all(), float(gap.min())
    for p in c["equal_rows"]:
        assert np.array_equal(ref["frame64"][:, :, p], np.zeros((L, H), np.int32))
        assert np.allclose(ref["peak64"][:, :, p], 1 / F, rtol=1e-14)
    for p, where in c["ties"]:
        kk = k[list(where), :, 0]
        assert all(np.array_equal(kk[0].view(np.uint32), x.view(np.uint32)) for x in kk[1:])
        assert (ref["frame64"][:, :, p] == min(where)).all()


def test_big_cases_would_overflow_without_the_running_maximum():
    """the scores go beyond 80 and a float32 sum of exp(s) over the row is infinite in some rows"""
    assert max(HC.reference(n)["smax"] for n in HC.NAMES) >= 80
    overflowing = 0
    for n in HC.NAMES:
        with np.errstate(over="ignore"):
            naive = np.exp(HR.scores(HC.case(n)).astype(np.float32)).sum(-1, dtype=np.float32)
        overflowing += int(np.isinf(naive).sum())
    assert overflowing >= 10, overflowing


def test_fold_clip_is_the_scripts_arithmetic():
    rng = np.random.default_rng(5)
    peaks = rng.uniform(0.001, 0.9, (3, 4, 17)).astype(np.float32)
    peaks[0, 1] = 0.25                      # a constant row: deviation 0, the 1e-6 decides, no vote
    peaks[1, 2] = 0.01
    peaks[1, 2, 5] = 0.9                    # one outlier among 17: z = 4 > 3
    peaks[2, 0, :] = np.linspace(0.1, 0.2, 17, dtype=np.float32)
    strength, vote = AH.fold_clip(peaks)
    t = torch.from_numpy(peaks).double()    # determine_alignment_heads.py:168-174, per layer
    for l in range(3):
        peak = t[l]
        want_strength = peak.mean(dim=-1)
        z = (peak - peak.mean(dim=-1, keepdim=True)) / (peak.std(dim=-1, keepdim=True, unbiased=False) + 1e-6)
        want_vote = (z > 3).any(dim=-1)
        assert np.allclose(strength[l], want_strength.numpy(), rtol=1e-14, atol=0)
        assert np.array_equal(vote[l], want_vote.numpy())
    assert not vote[0, 1] and vote[1, 2] and not vote[2, 0]
    assert strength.dtype == np.float64 and vote.dtype == np.bool_
    assert AH.fold_clip(peaks, z_threshold=5.0)[1].sum() == 0


def test_select_heads_rules():
    s = np.array([[0.05, 0.0501], [0.3, 0.0]])
    v = np.array([[1.0, 0.5], [0.4, 0.51]])
    assert AH.select_heads(s).tolist() == [[False, True], [True, False]]
    assert AH.select_heads(s, v, min_votes=0.5).tolist() == [[True, False], [False, True]]
    assert AH.select_heads(s, min_strength=0.2).tolist() == [[False, False], [True, False]]
    with pytest.raises(ValueError):
        AH.select_heads(s, min_votes=0.5)


def test_load_mask_reproduces_every_head_table():
    with open(os.path.join(GOLDEN, "alignment_head_dumps.json")) as fh:
        dumps = json.load(fh)
    with open(os.path.join(GOLDEN, "alignment_heads.json")) as fh:
        pairs = json.load(fh)
    assert set(dumps) == set(pairs) and len(dumps) >= 10
    for name, dump in dumps.items():
        got = AH.mask_pairs(AH.load_mask(dump, MODEL_DIMS[name]))
        assert got == [tuple(p) for p in pairs[name]] == list(ALIGNMENT_HEADS[name]), name
        assert AH.mask_pairs(AH.load_mask(dump.encode(), MODEL_DIMS[name])) == got


def test_dump_round_trip_and_refusals():
    rng = np.random.default_rng(2)
    for shape in ((2, 2), (6, 8), (32, 20)):
        mask = rng.random(shape) < 0.1
        dims = type("D", (), dict(n_text_layer=shape[0], n_text_head=shape[1]))
        text = AH.dump_mask(mask)
        assert isinstance(text, str) and text.isascii()
        back = AH.load_mask(text + "\n", dims)          # as read from the file the command line writes
        assert back.dtype == np.bool_ and np.array_equal(back, mask)
        assert AH.mask_pairs(back) == [(int(l), int(h)) for l, h in np.argwhere(mask)]
    with pytest.raises(ValueError):
        AH.load_mask(AH.dump_mask(np.zeros((2, 2), bool)), MODEL_DIMS["tiny"])
    with pytest.raises(ValueError):
        AH.dump_mask(np.zeros(4, bool))


def test_custom_alignment_heads_string_resolves_to_the_pairs():
    dims = MODEL_DIMS["base.en"]
    pairs = list(ALIGNMENT_HEADS["base.en"])
    mask = np.zeros((dims.n_text_layer, dims.n_text_head), bool)
    for l, h in pairs:
        mask[l, h] = True
    assert AH.resolve_custom_heads(AH.dump_mask(mask), dims) == pairs
    assert AH.resolve_custom_heads(pairs, dims) == pairs
    assert AH.resolve_custom_heads([[3, 3], [4, 7]], dims) == [(3, 3), (4, 7)]
    assert AH.resolve_custom_heads(None, dims) is None and AH.resolve_custom_heads([], dims) is None


def test_survey_tokens_layout():
    tok = type("T", (), dict(sot_sequence=(7, 8, 9), no_timestamps=11, eot=5, encode=staticmethod(lambda text: [len(text), 2])))
    assert AH.survey_tokens(tok, "abcd") == [7, 8, 9, 11, 4, 2, 5]


def test_pad_or_trim_audio():
    a = np.arange(10, dtype=np.float32)
    assert np.array_equal(AH.pad_or_trim_audio(a, 4), a[:4])
    assert np.array_equal(AH.pad_or_trim_audio(a, 12), np.concatenate([a, np.zeros(2, np.float32)]))
    assert AH.pad_or_trim_audio(a).shape == (480000,)


def test_planted_heads_on_the_cpu_oracle():
    """what the GPU test relies on: planted heads at strength >= 0.2, every other head <= 0.0125 (4 x away from the 0.05
    rule on either side), for each of the three seeded clips"""
    dims, sd = HC.planted_state_dict()
    assert (dims.n_text_layer, dims.n_text_head) == (2, 2)
    from whisperlivekit_amd.tokenizer import get_tokenizer
    tok = HC.PlantedTokenizer
    cli_tok = get_tokenizer(dims.is_multilingual, num_languages=dims.num_languages, language="en", task="transcribe", synthetic=True)
    for seed, text in [(0, None), (1, None), (2, None), (0, HC.CLI_TEXT), (1, HC.CLI_TEXT)]:
        audio, transcript = HC.planted_clip(seed)
        tokens = AH.survey_tokens(tok, transcript) if text is None else AH.survey_tokens(cli_tok, text)
        if text is None:
            assert tokens[:4] == [*tok.sot_sequence, tok.no_timestamps] and tokens[-1] == tok.eot and len(tokens) == 19
        assert 3 < len(tokens) <= dims.n_text_ctx and max(tokens) < dims.n_vocab
        _, peaks = HC.oracle_peaks(sd, dims, HC.oracle_log_mel(audio, dims.n_mels), tokens)
        strength, _ = AH.fold_clip(peaks)
        print(seed, strength.tolist())
        for l in range(2):
            for h in range(2):
                if (l, h) in HC.PLANTED:
                    assert strength[l, h] >= 0.2, (seed, l, h, strength[l, h])
                else:
                    assert strength[l, h] <= 0.0125, (seed, l, h, strength[l, h])
        assert AH.mask_pairs(AH.select_heads(strength)) == sorted(HC.PLANTED)
