#!/usr/bin/env python
"""Word alignment of concurrent greedy `transcribe(word_timestamps=True)` calls on one model: stack on and the alignment
switch off (every window's `find_alignment` on its own session: the parent behaviour, the yardstick) against the switch on
(the windows of the calls in flight share one stacked alignment pass).

    align_stack_probe.py [model=base.en] [--calls 1,2,4,8] [--stack 8] [--pairs 3] [--seconds 30] [--tokens 100] [--repeat 3]

Part 1, the leg alone: one encoded session per window, a window of `tokens` text tokens over the whole 30 s; after a
warm-up, alternating pairs of (n solo `timing.find_alignment` calls one after the other, ONE `find_alignment_many` of the n
windows); medians and the spread of the pairs, in ms per window.  n = 1 is the decision "does a lone window take the
group": it does unless the group of one is slower than the solo call outside the spread of the pairs.
Part 2, the calls: per number of concurrent callers one warm-up of each mode, then alternating (off, on) runs; every caller
transcribes its own recording `repeat` times, each as one window of `tokens` greedy steps (random weights end a window
within two steps, so <|endoftext|> is suppressed and the window runs to sample_len; no timestamps: one window per
recording).  Printed per run: ms per call, audio-s/s over all calls, the alignment leg's ms per window as the callers see it
(wall time inside the alignment call, queueing included) and the windows per stacked pass."""
import argparse
import os
import statistics
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("WLK_SYNTHETIC_VOCAB", "1")
import numpy as np  # noqa: E402

from whisperlivekit_amd import synth, timing  # noqa: E402
from whisperlivekit_amd import transcribe as TR  # noqa: E402
from whisperlivekit_amd.engine import HipWhisperModel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("model", nargs="?", default="base.en")
ap.add_argument("--calls", default="1,2,4,8")
ap.add_argument("--stack", type=int, default=8)
ap.add_argument("--pairs", type=int, default=3)
ap.add_argument("--seconds", type=float, default=30.0)
ap.add_argument("--tokens", type=int, default=100)
ap.add_argument("--repeat", type=int, default=3)
args = ap.parse_args()
counts = [int(x) for x in args.calls.split(",")]

model = HipWhisperModel.synthetic(args.model, 0, device=0)
tok = TR._tokenizer_for(model, "en", "transcribe")
audios = [synth.speech_like(args.seconds, seed=i) for i in range(8)]
num_frames = int(args.seconds * 100)
TR.set_stack(model, args.stack)
group = TR.window_stacker(model, args.stack).group

# ---- part 1: the alignment leg alone ---------------------------------------------------------------------------------------------
sessions = []
for i in range(max(counts)):
    s = model.new_session(beam=1, max_audio_seconds=31.0, batched=False)
    s.encode_mel(TR.pad_or_trim(s.log_mel(audios[i])))
    sessions.append(s)
texts = [np.random.default_rng(i).integers(0, tok.eot, args.tokens).tolist() for i in range(max(counts))]
n_tokens = len(tok.sot_sequence) + 2 + args.tokens
print(f"{args.model}: the alignment leg alone, {args.tokens} text tokens over {num_frames} frames per window; "
      f"fits the stacked pass: {group.fits(n_tokens, num_frames)}; {2 * args.pairs + 1} alternating pairs")
print(f"{'windows':>7} {'solo ms/window':>15} {'(min .. max)':>18} {'group ms/window':>16} {'(min .. max)':>18}")


def leg(n, stacked):
    a = time.perf_counter()
    if stacked:
        got = timing.find_alignment_many(group, [(sessions[i], tok, texts[i], num_frames) for i in range(n)])
    else:
        got = [timing.find_alignment(sessions[i], tok, texts[i], None, num_frames) for i in range(n)]
    return (time.perf_counter() - a) * 1e3 / n, got


for n in counts:
    (_t, a), (_t, b) = leg(n, False), leg(n, True)
    same = [[(w.word, w.start, w.end, w.probability) for w in x] for x in a] == [[(w.word, w.start, w.end, w.probability) for w in x] for x in b]
    solo, grp = [], []
    for _pair in range(2 * args.pairs + 1):
        solo.append(leg(n, False)[0])
        grp.append(leg(n, True)[0])
    print(f"{n:>7} {statistics.median(solo):15.3f} {'(%.3f .. %.3f)' % (min(solo), max(solo)):>18} {statistics.median(grp):16.3f} "
          f"{'(%.3f .. %.3f)' % (min(grp), max(grp)):>18}   same words: {same}")
for s in sessions:
    s.close()

# ---- part 2: concurrent transcribe calls ------------------------------------------------------------------------------------------
kw = dict(language="en", temperature=0.0, sample_len=args.tokens, suppress_tokens=f"-1,{tok.eot}", without_timestamps=True,
          logprob_threshold=None, compression_ratio_threshold=None, no_speech_threshold=None, word_timestamps=True)
leg_ms = []
leg_lock = threading.Lock()


def timed(fn):
    def wrapper(*a, **k):
        t0 = time.perf_counter()
        try:
            return fn(*a, **k)
        finally:
            with leg_lock:
                leg_ms.append((time.perf_counter() - t0) * 1e3)
    return wrapper


solo_find_alignment = timing.find_alignment
TR.AlignStacker.align = timed(TR.AlignStacker.align)


def run(n_calls, align):
    """-> (wall seconds, alignment ms per window, windows per stacked pass or None, the callers' results)"""
    TR.set_align_stack(model, align)
    # with the switch on the solo call is reached only from inside the stacker (already timed there)
    timing.find_alignment = solo_find_alignment if align else timed(solo_find_alignment)
    st = TR.align_stacker(model)
    before = st.stats() if st is not None else None
    del leg_ms[:]
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
    per_pass = None
    st = TR.align_stacker(model)
    if align and st is not None:
        after = st.stats()
        passes = after["group_passes"] - (before["group_passes"] if before else 0)
        per_pass = (after["stacked"] - (before["stacked"] if before else 0)) / max(passes, 1)
    return wall, statistics.mean(leg_ms) if leg_ms else float("nan"), per_pass, out


print(f"\n{args.model}: {args.seconds:.0f} s recordings x {args.repeat} per caller, {args.tokens} greedy steps per window, "
      f"stack = {args.stack} rows in both modes, {args.pairs} alternating pairs")
print(f"{'calls':>5} {'align':>6} {'ms/call':>9} {'audio-s/s':>10} {'align ms/window':>16} {'windows/pass':>13}")
for n in counts:
    run(n, False)
    run(n, True)
    same = True
    rows = {False: [], True: []}
    for _pair in range(args.pairs):
        ref = None
        for align in (False, True):
            wall, ms, per_pass, out = run(n, align)
            same = same and (ref is None or ref == out)
            ref = out
            rows[align].append((wall * 1e3 / args.repeat, n * args.repeat * args.seconds / wall, ms))
            print(f"{n:>5} {'on' if align else 'off':>6} {wall * 1e3 / args.repeat:9.2f} {n * args.repeat * args.seconds / wall:10.1f} "
                  f"{ms:16.3f} {('%.2f' % per_pass) if per_pass else '-':>13}")
    med = {k: [statistics.median(col) for col in zip(*v)] for k, v in rows.items()}
    print(f"{n:>5} medians: off {med[False][0]:.2f} ms/call {med[False][1]:.1f} audio-s/s {med[False][2]:.3f} ms/window | "
          f"on {med[True][0]:.2f} ms/call {med[True][1]:.1f} audio-s/s {med[True][2]:.3f} ms/window; same results: {same}")
TR.release_sessions(model)
model.close()
