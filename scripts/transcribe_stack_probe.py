#!/usr/bin/env python
"""Concurrent greedy `transcribe()` calls on one model, stack off (every call drives its own one-row step chain: the parent
behaviour, the yardstick) against stack on (the steps of the calls in flight share one window-group chain).

    transcribe_stack_probe.py [model=base.en] [--calls 1,2,4,8] [--stack 8] [--pairs 3] [--seconds 30] [--tokens 100]
                              [--repeat 5]

Per number of concurrent calls: one warm-up of each mode, then `pairs` alternating (off, on) runs.  Every caller transcribes
its own 30 s recording `repeat` times in a row, each time as one window of `tokens` greedy steps at temperature 0 (random
weights end a window within two steps, so <|endoftext|> is suppressed and the window runs to sample_len; no timestamps: one
window per recording).
Printed per run: wall time, ms per decoder step as one caller sees it (wall / steps of one caller), rows per group step
(stack on: from the group's counters), audio-s/s over all calls."""
import argparse
import os
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("WLK_SYNTHETIC_VOCAB", "1")
from whisperlivekit_amd import synth  # noqa: E402
from whisperlivekit_amd import transcribe as TR  # noqa: E402
from whisperlivekit_amd.engine import HipWhisperModel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("model", nargs="?", default="base.en")
ap.add_argument("--calls", default="1,2,4,8")
ap.add_argument("--stack", type=int, default=8)
ap.add_argument("--pairs", type=int, default=3)
ap.add_argument("--seconds", type=float, default=30.0)
ap.add_argument("--tokens", type=int, default=100)
ap.add_argument("--repeat", type=int, default=5)
args = ap.parse_args()

model = HipWhisperModel.synthetic(args.model, 0, device=0)
eot = TR._tokenizer_for(model, "en", "transcribe").eot
kw = dict(language="en", temperature=0.0, sample_len=args.tokens, suppress_tokens=f"-1,{eot}", without_timestamps=True,
          logprob_threshold=None, compression_ratio_threshold=None, no_speech_threshold=None)
audios = [synth.speech_like(args.seconds, seed=i) for i in range(8)]


def run(n_calls, stack):
    """-> (wall seconds, steps of one caller, rows per group step or None, the callers' token lists)"""
    TR.set_stack(model, stack)
    st = TR.window_stacker(model)
    before = st.stats() if st is not None else None
    out = [None] * n_calls
    start = threading.Barrier(n_calls + 1)

    def work(i):
        start.wait()
        for _rep in range(args.repeat):
            out[i] = TR.transcribe(model, audios[i], **kw)
    ts = [threading.Thread(target=work, args=(i,)) for i in range(n_calls)]
    for t in ts:
        t.start()
    start.wait()
    a = time.perf_counter()
    for t in ts:
        t.join()
    wall = time.perf_counter() - a
    if any(o is None for o in out):
        raise RuntimeError("a transcribe() call failed")
    rows = None
    st = TR.window_stacker(model)
    if stack and st is not None:
        after = st.stats()
        steps = after["steps"] - (before["steps"] if before else 0)
        rows = (after["rows"] - (before["rows"] if before else 0)) / max(steps, 1)
    tokens = [[t for s in o["segments"] for t in s["tokens"]] for o in out]
    return wall, len(tokens[0]) * args.repeat, rows, tokens


print(f"{args.model}: {args.seconds:.0f} s recordings x {args.repeat} per caller, {args.tokens} greedy steps per window, "
      f"stack = {args.stack} rows, {args.pairs} alternating pairs")
print(f"{'calls':>5} {'mode':>9} {'wall s':>8} {'ms/step':>8} {'rows/group step':>16} {'audio-s/s':>10}")
for n in [int(x) for x in args.calls.split(",")]:
    run(n, 0)
    run(n, args.stack)
    same = True
    for _pair in range(args.pairs):
        ref = None
        for mode, stack in (("stack off", 0), ("stack on", args.stack)):
            wall, steps, rows, tokens = run(n, stack)
            same = same and (ref is None or ref == tokens)
            ref = tokens
            print(f"{n:>5} {mode:>9} {wall:8.3f} {wall * 1e3 / max(steps, 1):8.3f} {('%.2f' % rows) if rows else '-':>16} "
                  f"{n * args.repeat * args.seconds / wall:10.1f}")
    print(f"{n:>5} same tokens in both modes: {same}")
TR.release_sessions(model)
model.close()
