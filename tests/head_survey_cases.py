"""Inputs of the alignment-head survey tests: one generator module for test_head_survey_cpu.py (which checks the references
and the generator's own conditions on these very cases) and test_gpu_head_survey.py (which runs them through
wlk_diag_head_survey).  Seeded by name.

A kernel case: q [n_layer][P][d] (d = 64 n_head, the scaled queries), k [Tk][n_layer 2 d] in the session's cross K|V layout
(ldkv = n_layer 2 d as in production; the V halves and every row at or beyond F hold NaN), F <= Tk.  The largest score of
a "big" case is +95 (none beyond 100 in magnitude: asserted), so a sum without the running maximum overflows.
Conditions the generator enforces and the CPU test asserts: in float64 the top score of every row leads the runner-up
among distinct keys by >= 1e-3 (a row that misses it has its QUERY nudged along its top key - a query row belongs to one
score row only, a key to all P of them); `dups` lists the positions that repeat an earlier key row bit for bit (the tie
plants), `equal_rows` the query rows that are all zero (every score equal: peak 1 / F, frame 0).

The model case (planted heads): micro (2 layers x 2 heads), synth_state_dict(dims, 3) with the rows of
cross_attn.query.weight / .bias of heads (0, 1) and (1, 0) multiplied by a gain.  With a Gaussian mel a gain of 8 already
separates them (strengths 0.4 / 0.3 against 0.004); collect_heads starts from AUDIO, and on the log-mel of the seeded
speech-like clips used here a gain of 8 leaves head (1, 0) at 0.06 - 0.11, so the fixture takes 24 (0.39 - 0.60 against
0.0025 on the CPU oracle; test_head_survey_cpu.py asserts >= 0.2 and <= 0.0125 for every clip)."""
import functools

import numpy as np

from dec_attention_cases import hash_name

import head_survey_reference as HR

GAP = 1e-3
TRIP = 128           # keys per staging trip of the kernel: a key range is whole trips


def _rng(name):
    return np.random.default_rng(hash_name(name))


def max_splits(F):
    return (F + TRIP - 1) // TRIP


def make(name, L, H, P, F, Tk, style="big", ties=(), equal_rows=(), dominant=()):
    """ties: (query row, [key positions]) - the keys at those positions become one bit-identical row that dominates that
    query row in every (layer, head); dominant: (query row, key position) the same with a single key"""
    rng = _rng(name)
    d = 64 * H
    amp = 1.5 if style == "big" else 0.4
    q = (rng.standard_normal((L, P, d)) * amp).astype(np.float32)
    k = np.full((Tk, L, 2, H, 64), np.nan, np.float32)
    k[:F, :, 0] = (rng.standard_normal((F, L, H, 64)) * amp).astype(np.float32)
    if style == "big":      # the largest |score| of the case: 95, and positive (exp(95) is infinite in float32)
        k64 = k[:F, :, 0].astype(np.float64)
        s = np.einsum("lphk,flhk->lhpf", q.reshape(L, P, H, 64).astype(np.float64), k64)
        top = s.flat[np.abs(s).argmax()]
        q = (q * (95.0 / top)).astype(np.float32)
    for p in equal_rows:
        q[:, p] = 0
    dups = []
    for p, where in list(ties) + [(p, [f]) for p, f in dominant]:
        qp = q[:, p].reshape(L, H, 64).astype(np.float64)
        row = (qp * (80.0 / (qp * qp).sum(-1, keepdims=True))).astype(np.float32)       # q . row = 80
        for f in where:
            k[f, :, 0] = row
        dups += sorted(where)[1:]
    c = dict(name=name, n_layer=L, n_head=H, P=P, F=F, Tk=Tk, ldq=d, ldkv=L * 2 * d, q=q, k=k.reshape(Tk, L * 2 * d),
             dups=tuple(sorted(dups)), equal_rows=tuple(equal_rows), ties=tuple((p, tuple(w)) for p, w in ties))
    # the lead of the top score: nudge the query of a row that misses it along its top key (float32 data, float64 check)
    for _ in range(20):
        s = HR.scores(c)
        gap = HR.top_gap(s, c["dups"])
        gap[:, :, list(equal_rows)] = np.inf
        bad = np.argwhere(gap < 2 * GAP) if F > 1 else []
        if len(bad) == 0:
            break
        kk = c["k"].reshape(Tk, L, 2, H, 64)
        for l, h, p in bad:
            top = kk[int(s[l, h, p].argmax()), l, 0, h].astype(np.float64)
            qq = q[l, p, 64 * h:64 * h + 64].astype(np.float64) + top * (8 * GAP / (top * top).sum())
            q[l, p, 64 * h:64 * h + 64] = qq.astype(np.float32)
    return c


def _specs():
    out = {}

    def add(name, *a, **kw):
        out[name] = (a, kw)

    Ps, Hs, Ls = (1, 31, 32, 33, 70), (1, 2, 20), (1, 3)
    for i, F in enumerate((1, 3, 63, 64, 65, 127, 129, 1500)):          # every F, the other axes cycling
        P, H, L = Ps[i % 5], Hs[i % 3], Ls[i % 2]
        Tk = (F, F + 5, 1500)[i % 3]
        add(f"f{F}_p{P}_h{H}_l{L}_tk{Tk}", L, H, P, F, Tk)
    for i, P in enumerate(Ps):                                          # every P at a short and at the full key count
        F = (129, 1500)[i % 2]
        add(f"p{P}_f{F}_h{Hs[(i + 1) % 3]}_l{Ls[(i + 1) % 2]}", Ls[(i + 1) % 2], Hs[(i + 1) % 3], P, F, (F + 5, 1500)[i % 2])
    add("heads20_layers3_p33_f1500", 3, 20, 33, 1500, 1500)            # 120 (layer, head) pairs x 2 query tiles
    add("heads20_p70_f129", 1, 20, 70, 129, 134)
    add("small_scores_p33_f200", 3, 2, 33, 200, 205, style="small")
    add("equal_and_dominant_f1500", 1, 2, 33, 1500, 1500, style="small", equal_rows=(0, 32), dominant=((1, 777), (31, 0), (2, 1499)))
    add("equal_and_dominant_f65", 3, 1, 5, 65, 70, style="small", equal_rows=(4,), dominant=((0, 64),))
    # bit-identical key rows: in one lane (1, 2), in the two halves of a wave (10, 14), in two waves of a trip (20, 52), in
    # one wave's two trips (30, 158), a later wave of an earlier trip (100, 130), in two key ranges (60, 1000), (700, 1499)
    add("ties_f1500", 1, 2, 33, 1500, 1500, style="small",
        ties=((0, (1, 2)), (1, (10, 14)), (2, (20, 52)), (3, (30, 158)), (4, (100, 130)), (5, (60, 1000)), (6, (700, 1499)),
              (32, (1300, 200, 650))))
    add("ties_f129", 3, 1, 5, 129, 129, style="small", ties=((0, (3, 128)), (1, (127, 128 - 32)), (4, (0, 5))))
    return out


SPECS = _specs()
NAMES = list(SPECS)


@functools.lru_cache(maxsize=None)
def case(name):
    a, kw = SPECS[name]
    return make(name, *a, **kw)


@functools.lru_cache(maxsize=None)
def reference(name):
    """computed once per session and shared: nobody writes into it"""
    ref = HR.reference(case(name))
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


# ---- planted heads ----------------------------------------------------------------------------------------------------
PLANTED = ((0, 1), (1, 0))
PLANT_SEED, PLANT_GAIN = 3, 24.0


@functools.lru_cache(maxsize=None)
def planted_state_dict():
    from whisperlivekit_amd import synth
    from whisperlivekit_amd.dims import MODEL_DIMS
    dims = MODEL_DIMS["micro"]
    sd = {k: np.array(v, copy=True) for k, v in synth.synth_state_dict(dims, PLANT_SEED).items()}
    for l, h in PLANTED:
        for part in ("weight", "bias"):
            w = np.array(sd[f"decoder.blocks.{l}.cross_attn.query.{part}"], np.float32, copy=True)
            w[64 * h:64 * h + 64] *= PLANT_GAIN
            sd[f"decoder.blocks.{l}.cross_attn.query.{part}"] = w
    return dims, sd


def planted_mel(seed):
    from whisperlivekit_amd.dims import MODEL_DIMS
    return np.random.default_rng(1000 + seed).standard_normal((MODEL_DIMS["micro"].n_mels, 3000)).astype(np.float32)


def planted_tokens(seed, n=14):
    return np.random.default_rng(2000 + seed).integers(0, 50000, n).astype(np.int64)


CLI_TEXT = "the quick brown fox jumps over the lazy dog"      # the command-line test's transcript (synthetic vocabulary)


def planted_clip(seed):
    """-> (16 kHz waveform, transcript): 4 s of seeded speech-like audio; the transcript names the seed of its tokens"""
    from whisperlivekit_amd import synth
    return synth.speech_like(4.0, seed), f"clip {seed}"


class PlantedTokenizer:
    """the four members collect_heads reads; encode() maps a planted_clip transcript to its seeded tokens"""
    sot_sequence, no_timestamps, eot = (50258, 50259, 50359), 50363, 50257

    @staticmethod
    def encode(text):
        return [int(t) for t in planted_tokens(int(text.split()[-1]))]


def oracle_log_mel(audio, n_mels):
    """whisper's log-mel of the clip padded to 30 s, on the CPU oracle -> [n_mels, 3000] float32"""
    import torch
    from oracle import whisper_oracle as wo
    from whisperlivekit_amd import alignment_heads as AH
    from whisperlivekit_amd.melbank import mel_filterbank
    mel = wo.log_mel_spectrogram(torch.from_numpy(AH.pad_or_trim_audio(audio)), torch.from_numpy(np.array(mel_filterbank(n_mels))))
    return np.ascontiguousarray(mel.numpy()[:, :3000], np.float32)


def oracle_peaks(sd, dims, mel, tokens, num_frames=3000, dtype=None):
    """the reference script's arithmetic on the CPU oracle: -> (scores [L, H, P, F] float64 as numpy, peaks [L, H, P])"""
    import torch
    from oracle import whisper_oracle as wo
    tsd = wo.to_torch_state_dict(sd)
    if dtype is not None:
        tsd = {k: v.to(dtype) for k, v in tsd.items()}
    with torch.no_grad():
        m = torch.from_numpy(mel)[None]
        enc = wo.encoder_forward(tsd, dims, m.to(dtype) if dtype is not None else m)
        _, qks = wo.decoder_forward(tsd, dims, torch.from_numpy(np.asarray(tokens, np.int64))[None], enc,
                                    wo.DecoderCache(dims.n_text_layer))
    s = torch.stack([qk[0] for qk in qks])[..., :num_frames // 2].double()
    return s.numpy(), s.softmax(-1).max(-1).values.numpy()
