#!/usr/bin/env python
"""Batch `decode()` of one 30 s window with beam search (beam_size 2, 5, 7) on seeded weights: the host beam path (logits of
every row read back per step, rules / log-softmax / top-k in numpy, wlk_kv_reorder) against the device path
(WLK_TRANSCRIBE_DEVICE_BEAM=1: wlk_pick_topk + wlk_decode_ancestry).  The two alternate on one box for three rounds after a
warm-up; per path: microseconds per decoder step (the window already encoded) and audio-seconds per second of the whole
call (encoder included)."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("WLK_SYNTHETIC_VOCAB", "1")
from whisperlivekit_amd import synth, transcribe as TR  # noqa: E402
from whisperlivekit_amd.engine import HipWhisperModel  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "base.en"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
model = HipWhisperModel.synthetic(name, 0, device=0)
audio = synth.speech_like(30.0, seed=0)
one = TR._rows_of(model).get(1)
mel = one.log_mel(audio, padding=TR.N_SAMPLES)
window = TR.pad_or_trim(mel[:, :TR.N_FRAMES])
PATHS = (("0", "host  "), ("1", "device"))


def counted(session):
    """Decoder forwards of `session` from here on (prefill, single-token steps of either kind)."""
    n = [0]
    for meth in ("decode", "decode_ancestry"):
        real = getattr(session, meth)
        setattr(session, meth, lambda *a, _real=real, **k: (n.__setitem__(0, n[0] + 1), _real(*a, **k))[1])
    return n


print(f"{name}, one 30 s window, seeded weights, {rounds} rounds after a warm-up; patience 2 keeps the search going")
for beam in (2, 5, 7):
    # seeded weights fill `finished` within a few tokens at patience 1: patience 2 makes the window a long decode
    kw = dict(language="en", temperature=0.0, beam_size=beam, patience=2.0)
    sess = TR._rows_of(model).get(beam)
    steps = counted(sess)
    results, step_us, rate = {}, {m: [] for m, _ in PATHS}, {m: [] for m, _ in PATHS}
    for rnd in range(rounds + 1):                       # round 0: warm-up (graph captures, allocations)
        for mode, _ in PATHS:
            os.environ["WLK_TRANSCRIBE_DEVICE_BEAM"] = mode
            a = time.perf_counter()
            res = TR.decode(model, window, **kw)
            full = time.perf_counter() - a
            steps[0] = 0
            a = time.perf_counter()
            TR.decode(model, None, session=sess, **kw)   # the window is encoded: decoder steps only
            dec = time.perf_counter() - a
            results[mode] = (res, steps[0], sess.beam_stats()["ancestry_steps"])
            if rnd > 0:
                step_us[mode].append(1e6 * dec / steps[0])
                rate[mode].append(30.0 / full)
    for mode, label in PATHS:
        res, n, anc = results[mode]
        print(f"beam {beam} {label}: {statistics.median(step_us[mode]):8.1f} us / decoder step "
              f"(rounds: {' '.join(f'{v:.1f}' for v in step_us[mode])}), {statistics.median(rate[mode]):7.1f} audio-s/s, "
              f"{n} steps, {len(res.tokens)} tokens, ancestry steps so far {anc}")
    h, d = results["0"][0], results["1"][0]
    print(f"beam {beam}: same tokens {h.tokens == d.tokens}, avg_logprob difference {abs(h.avg_logprob - d.avg_logprob):.2e}, "
          f"device / host step time {statistics.median(step_us['1']) / statistics.median(step_us['0']):.3f}")
TR.release_sessions(model)
model.close()
