#!/usr/bin/env python
"""The alignment-head survey against the nearest thing the library had before it: `wlk_head_survey` and
`wlk_find_alignment` on the same session and the same tokens (both make the teacher-forced prefill with the flash
cross-attention; find_alignment reads the model's ~10 alignment heads through the score window and runs the DTW, the survey
reads every head through head_survey_kernel).

    head_survey_probe.py [--models base.en,large-v3] [--tokens 60,448] [--pairs 7] [--trace]

After a warm-up of both calls at every shape: alternating (find_alignment, head_survey) pairs, host clock around calls
that end in a device synchronise; medians and the spread, in ms per call.  Per shape also the survey's launch geometry
(workgroups of the one launch against a launch per layer) and its score-equivalent work 2 L H P F 64 flop.
--trace: warm-up plus three surveys per shape and nothing else, for a `rocprofv3 --kernel-trace --stats` run of its own."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from whisperlivekit_amd import synth  # noqa: E402
from whisperlivekit_amd.engine import HipWhisperModel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--models", default="base.en,large-v3")
ap.add_argument("--tokens", default="60,448")
ap.add_argument("--pairs", type=int, default=7)
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()
NUM_FRAMES, F = 3000, 1500


def geometry(L, H, P):
    """launch_head_survey's own choice (csrc/head_survey.hip: head_survey_splits)"""
    tiles, trips = (P + 31) // 32, (F + 127) // 128
    groups = L * H * tiles
    want = 1 if groups >= 256 else min(-(-256 // groups), trips)
    per = -(-trips // want)
    return groups, -(-trips // per), H * tiles


for name in args.models.split(","):
    model = HipWhisperModel.synthetic(name, 0, device=0)
    d = model.dims
    multilingual = d.n_vocab >= 51865
    eot = 50257 if multilingual else 50256
    sot = [eot + 1, eot + 2, eot + 102] if multilingual else [eot + 1]
    sess = model.new_session(beam=1, max_audio_seconds=31.0, batched=False)
    mel = sess.log_mel(synth.speech_like(30.0, seed=1))[:, :3000]
    sess.encode_mel(np.ascontiguousarray(mel))
    for P in (int(x) for x in args.tokens.split(",")):
        P = min(P, d.n_text_ctx)
        n_text = P - len(sot) - 2
        tokens = [*sot, eot + 106, *np.random.default_rng(P).integers(0, eot, n_text).tolist(), eot]
        for _ in range(2):
            sess.find_alignment(tokens, len(sot), eot, NUM_FRAMES)
            sess.head_survey(tokens, NUM_FRAMES)
        if args.trace:
            for _ in range(3):
                sess.head_survey(tokens, NUM_FRAMES)
            continue
        t_fa, t_hs = [], []
        for _ in range(args.pairs):
            t0 = time.perf_counter()
            sess.find_alignment(tokens, len(sot), eot, NUM_FRAMES)
            t1 = time.perf_counter()
            sess.head_survey(tokens, NUM_FRAMES)
            t2 = time.perf_counter()
            t_fa.append((t1 - t0) * 1e3)
            t_hs.append((t2 - t1) * 1e3)
        groups, splits, per_layer = geometry(d.n_text_layer, d.n_text_head, P)
        flop = 2.0 * d.n_text_layer * d.n_text_head * P * F * 64
        print(f"{name} P={P}: find_alignment {statistics.median(t_fa):.3f} ms ({min(t_fa):.3f} .. {max(t_fa):.3f}) | "
              f"head_survey {statistics.median(t_hs):.3f} ms ({min(t_hs):.3f} .. {max(t_hs):.3f}) | {args.pairs} alternating pairs | "
              f"survey launch: {groups} x {splits} key ranges = {groups * splits} workgroups (a launch per layer: {per_layer}) | "
              f"{flop / 1e9:.3f} Gflop of scores, {len(model.alignment_heads)} alignment heads against "
              f"{d.n_text_layer * d.n_text_head} surveyed")
    sess.close()
    model.close()
