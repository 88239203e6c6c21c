"""Host-state vs device-state Sortformer sessions, same process, same model (full depth, synthetic weights): 30 s of
speech_like audio per session in 1 s chunks through HipSortformerDiarizationOnline, 1 session and 8 threaded sessions,
the two state kinds alternated over several rounds.  Prints p50 / p90 ms per chunk (wall time of diarize_sync) and the
stacked launch chains the run took.  Usage: python scripts/sf_state_probe.py [--rounds 3] [--seconds 30]"""
import argparse
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from whisperlivekit_amd import sortformer as sf  # noqa: E402
from whisperlivekit_amd.diarization import HipSortformerDiarizationOnline  # noqa: E402
from whisperlivekit_amd.synth import speech_like  # noqa: E402


def run(model, n_sess, on_device, seconds):
    audios = [speech_like(float(seconds), seed=100 + i).astype(np.float32) for i in range(n_sess)]
    onl = []
    for _ in range(n_sess):
        o = HipSortformerDiarizationOnline(model)
        if on_device:
            o.streaming_state = model.new_device_state()
        onl.append(o)
    times = [[] for _ in range(n_sess)]
    gate = threading.Barrier(n_sess)

    def worker(i):
        gate.wait()
        for k in range(seconds):
            onl[i].insert_audio_chunk(audios[i][k * 16000:(k + 1) * 16000])
            t0 = time.perf_counter()
            onl[i].diarize_sync()
            times[i].append((time.perf_counter() - t0) * 1e3)
    before = model.stats()
    th = [threading.Thread(target=worker, args=(i,)) for i in range(n_sess)]
    t0 = time.perf_counter()
    [t.start() for t in th]
    [t.join() for t in th]
    wall = time.perf_counter() - t0
    after = model.stats()
    for o in onl:
        o.close()
    ms = np.array([x for t in times for x in t[1:]])       # the first chunk of a session (12 rows, no context) left out
    return dict(p50=float(np.percentile(ms, 50)), p90=float(np.percentile(ms, 90)),
                stacked=after["stacked_steps"] - before["stacked_steps"], steps=after["session_steps"] - before["session_steps"],
                audio_s_per_s=n_sess * seconds / wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=int, default=30)
    a = ap.parse_args()
    model = sf.HipSortformerModel.synthetic(sf.SortformerDims(), seed=12)
    run(model, 1, False, 3)          # warm-up: kernels loaded, extractor built
    run(model, 1, True, 3)
    for r in range(a.rounds):
        for n in (1, 8):
            for dev in (False, True):
                x = run(model, n, dev, a.seconds)
                print(f"round {r} sessions {n} state {'device' if dev else 'host  '}  p50 {x['p50']:7.3f} ms  p90 {x['p90']:7.3f} ms"
                      f"  stacked steps {x['stacked']:4d} / session steps {x['steps']:4d}  {x['audio_s_per_s']:7.1f} audio-s/s",
                      flush=True)
    model.close()


if __name__ == "__main__":
    main()
