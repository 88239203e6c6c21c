#!/usr/bin/env python
"""Concurrent greedy `transcribe()` calls on one model, stack off (every call drives its own one-row step chain: the parent
behaviour, the yardstick) against stack on (the steps of the calls in flight share one window-group chain).

    transcribe_stack_probe.py [model=base.en] [--calls 1,2,4,8] [--stack 8] [--pairs 3] [--seconds 30] [--tokens 100]
                              [--repeat 5] [--burst 4,8,16] [--time-limit 360]

Per number of concurrent calls: one warm-up of each mode, then `pairs` alternating (off, on) runs.  Every caller transcribes
its own 30 s recording `repeat` times in a row, each time as one window of `tokens` greedy steps at temperature 0 (random
weights end a window within two steps, so <|endoftext|> is suppressed and the window runs to sample_len; no timestamps: one
window per recording).
Printed per run: wall time, ms per decoder step as one caller sees it (wall / steps of one caller), rows per group step
(stack on: from the group's counters), audio-s/s over all calls.

With --burst the table is the burst axis of DESIGN 28 instead: stack on in every arm, burst 1 (the parent's behaviour)
against each listed burst, plus a lone caller kept in the group (solo_single off).  Printed per run: ms per step, audio-s/s,
rows per launch chain and the share of enqueued row slots that rows which had ended took up."""
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
ap.add_argument("--burst", default="", help="e.g. 4,8,16: the burst table (steps per library call) instead of stack off / on")
ap.add_argument("--time-limit", type=float, default=360.0, help="burst table: seconds after which no further arm is started")
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


def burst_table():
    """The burst axis: stack on in every arm, burst 1 (one library call per token: the yardstick) against each
    burst of --burst in alternating pairs after a warm-up of both arms.  Arms that would start after --time-limit seconds
    are reported as not measured."""
    t0 = time.perf_counter()
    print(f"{args.model}: {args.seconds:.0f} s recordings x {args.repeat} per caller, {args.tokens} greedy steps per window, "
          f"stack = {args.stack} rows, bursts {args.burst} against burst 1, {args.pairs} alternating pairs")
    print(f"{'calls':>5} {'arm':>22} {'wall s':>8} {'ms/step':>8} {'audio-s/s':>10} {'rows/chain':>11} {'dead slots':>11}")
    arms = [(n, k, True) for n in [int(x) for x in args.calls.split(",")] for k in [int(x) for x in args.burst.split(",")]]
    arms += [(1, k, False) for k in [int(x) for x in args.burst.split(",")]]      # a lone caller kept in the group
    for n, k, solo_single in arms:
        label = f"burst {k}" + ("" if solo_single else ", solo_single off")
        if time.perf_counter() - t0 > args.time_limit:
            print(f"{n:>5} {label:>22} not measured (time limit)")
            continue
        TR.set_stack(model, args.stack)
        TR.window_stacker(model, args.stack).solo_single = solo_single

        def arm(burst):
            TR.set_burst(model, burst)
            st = TR.window_stacker(model)
            before = st.stats()
            wall, steps, _rows, tokens = run(n, args.stack)
            after = st.stats()
            chains, rows, slots = (after[f] - before[f] for f in ("steps", "rows", "row_slots"))
            return wall, steps, tokens, (rows / chains if chains else None), (1.0 - rows / slots if slots else None)
        arm(1)
        arm(k)
        same = True
        for _pair in range(args.pairs):
            ref = None
            for burst in (1, k):
                wall, steps, tokens, per_chain, dead = arm(burst)
                same = same and (ref is None or ref == tokens)
                ref = tokens
                name = label if burst == k else "burst 1" + ("" if solo_single else ", solo_single off")
                print(f"{n:>5} {name:>22} {wall:8.3f} {wall * 1e3 / max(steps, 1):8.3f} {n * args.repeat * args.seconds / wall:10.1f} "
                      f"{('%.2f' % per_chain) if per_chain else '-':>11} {('%.1f %%' % (100 * dead)) if dead is not None else '-':>11}")
        print(f"{n:>5} same tokens in all arms: {same}")
    TR.window_stacker(model).solo_single = True
    TR.set_burst(model, None)


if args.burst:
    burst_table()
    TR.release_sessions(model)
    model.close()
    sys.exit(0)

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
