#!/usr/bin/env python
"""Beam streams, per-token path against the library loop (wlk_decode_beam_until_stop), on ONE box: base.en seeded
weights, one 30 s synthetic stream in 0.5 s chunks, beams 2 / 3 / 5, the two paths alternating, three rounds after one
warm-up round.  Per (beam, path): p50 ms per process_iter, microseconds per decode step (all process_iter wall time over the
decoder forwards run, so the encoder's share is in it on both sides), audio-s/s; and whether both paths took the same
decisions.  GPU box only."""
import os
import statistics
import sys
import time

os.environ.setdefault("WLK_SYNTHETIC_VOCAB", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from whisperlivekit_amd import synth  # noqa: E402
from whisperlivekit_amd.backend import HipSimulStreamingASR, HipSimulStreamingOnlineProcessor  # noqa: E402
from whisperlivekit_amd.engine import HipWhisperModel  # noqa: E402

SECONDS, CHUNK, ROUNDS = 30.0, 8000, 3
model = HipWhisperModel.synthetic("base.en", 0)
audio = synth.to_pcm16_roundtrip(synth.speech_like(SECONDS, 0))


def stream(beams, loop):
    asr = HipSimulStreamingASR("base.en", hip_model=model, beams=beams)
    proc = HipSimulStreamingOnlineProcessor(asr)
    m = proc.model
    m.use_beam_loop = loop
    m.decision_log = []
    assert m.beam_loop_available() == loop
    iters = []
    t_all = time.perf_counter()
    for lo in range(0, len(audio), CHUNK):
        hi = min(lo + CHUNK, len(audio))
        proc.insert_audio_chunk(audio[lo:hi].copy(), hi / 16000)
        t0 = time.perf_counter()
        proc.process_iter()
        iters.append(time.perf_counter() - t0)
    wall = time.perf_counter() - t_all
    steps = m.counters["decode"]
    log = [[c, [(int(t), int(f)) for t, f in s]] for c, s in m.decision_log]
    anc = m.session.beam_stats()["ancestry_steps"]
    proc.close()
    return dict(p50_ms=statistics.median(iters) * 1e3, us_per_step=sum(iters) / max(steps, 1) * 1e6, steps=steps,
                audio_s_per_s=SECONDS / wall, log=log, ancestry_steps=anc)


print(f"# beam loop probe: base.en seeded weights, {SECONDS:.0f} s stream, {CHUNK / 16000:.1f} s chunks, "
      f"{ROUNDS} rounds after a warm-up round, paths alternating", flush=True)
for beams in (2, 3, 5):
    for loop in (False, True):
        stream(beams, loop)                                   # warm-up: graph captures, allocator
    rows = {False: [], True: []}
    for rnd in range(ROUNDS):
        for loop in (False, True):
            r = stream(beams, loop)
            rows[loop].append(r)
            print(f"beam {beams} round {rnd} {'loop     ' if loop else 'per-token'}: p50 {r['p50_ms']:7.2f} ms/process_iter  "
                  f"{r['us_per_step']:8.1f} us/decode step ({r['steps']} steps, {r['ancestry_steps']} over the ancestry table)  "
                  f"{r['audio_s_per_s']:6.2f} audio-s/s", flush=True)
    same = all(a["log"] == b["log"] for a, b in zip(rows[False], rows[True]))
    med = lambda loop, k: statistics.median(r[k] for r in rows[loop])
    print(f"beam {beams} median: per-token p50 {med(False, 'p50_ms'):.2f} ms, {med(False, 'us_per_step'):.1f} us/step, "
          f"{med(False, 'audio_s_per_s'):.2f} audio-s/s | loop p50 {med(True, 'p50_ms'):.2f} ms, {med(True, 'us_per_step'):.1f} us/step, "
          f"{med(True, 'audio_s_per_s'):.2f} audio-s/s | speed-up {med(True, 'audio_s_per_s') / med(False, 'audio_s_per_s'):.3f}x | "
          f"decisions identical: {same}", flush=True)
model.close()
