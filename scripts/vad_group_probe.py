"""Time one tick of the VAD gate for 8 sessions (config 4, VAC on): eight wlk_vad_stream_run calls against one
wlk_vad_group_run, for fp32 and for int16 input.  8 streams x 16 windows per tick, 200 ticks per arm; the four arms run
one after the other and the whole set repeats, so that each arm is seen several times on the same box.
Host clock around calls that end in a stream synchronise.  `--arms solo_f32` needs nothing of the group, so the same
file also times a checkout that predates it (the comparison with the parent commit)."""
import argparse
import ctypes as C
import sys
import time

import numpy as np

ROOT = __file__.rsplit("/scripts/", 1)[0]
sys.path.insert(0, ROOT)
from whisperlivekit_amd import _lib, synth, vad as V  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=8)
ap.add_argument("--windows", type=int, default=16)
ap.add_argument("--ticks", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--arms", default="solo_f32,group_f32,solo_s16,group_s16")
args = ap.parse_args()
S, NW, T = args.streams, args.windows, args.ticks
N = NW * 512

lib = _lib.load()
flat = V.pack_vad_weights(dict(np.load(ROOT + "/tests/golden/vad_weights_16k.npz")))
# every stream its own speech-like audio (20 ticks of it, repeated); one tick of all streams lies back to back, as a
# group call takes it
CLIP = 20
f32 = np.stack([synth.to_pcm16_roundtrip(synth.speech_like(CLIP * N / 16000.0 + 0.1, seed))[: CLIP * N].reshape(CLIP, N)
                for seed in range(S)], axis=1)
f32 = np.ascontiguousarray(np.tile(f32, (-(-T // CLIP), 1, 1))[:T])                # [tick, stream, sample]
s16 = np.round(f32 * 32768.0).astype(np.int16)
assert np.array_equal(s16.astype(np.float32) / np.float32(32768.0), f32)
ptr = lambda a: a.ctypes.data_as(C.c_void_p)
print("audio ready", f32.shape, float(np.abs(f32).max()), flush=True)
wh = C.c_void_p()
_lib.check(lib.wlk_vad_create(0, flat.ctypes.data_as(C.c_void_p), flat.size, C.byref(wh)))


def new_streams():
    hs = []
    for _ in range(S):
        h = C.c_void_p()
        _lib.check(lib.wlk_vad_stream_create(wh, NW, C.byref(h)))
        hs.append(h)
    return hs


def run_solo(data, fn):
    hs, out, us = new_streams(), np.empty((T, S, NW), np.float32), np.empty(T)
    for t in range(T):
        t0 = time.perf_counter()
        for i in range(S):
            rc = fn(hs[i], ptr(data[t, i]), NW, ptr(out[t, i]))
            if rc:
                _lib.check(rc)
        us[t] = 1e6 * (time.perf_counter() - t0)
    for h in hs:
        lib.wlk_vad_stream_destroy(h)
    return out, us


def run_group(data, fmt):
    hs, out, us = new_streams(), np.empty((T, S, NW), np.float32), np.empty(T)
    g = C.c_void_p()
    _lib.check(lib.wlk_vad_group_create(wh, S, S * NW, C.byref(g)))
    handles = (C.c_void_p * S)(*hs)
    counts = (C.c_int32 * S)(*([NW] * S))
    for t in range(T):
        t0 = time.perf_counter()
        rc = lib.wlk_vad_group_run(g, handles, counts, S, ptr(data[t]), fmt, ptr(out[t]))
        us[t] = 1e6 * (time.perf_counter() - t0)
        if rc:
            _lib.check(rc)
    lib.wlk_vad_group_destroy(g)
    for h in hs:
        lib.wlk_vad_stream_destroy(h)
    return out, us


arms = {"solo_f32": lambda: run_solo(f32, lib.wlk_vad_stream_run), "group_f32": lambda: run_group(f32, 0),
        "solo_s16": lambda: run_solo(s16, lib.wlk_vad_stream_run_pcm16), "group_s16": lambda: run_group(s16, 1)}
arms = [(name, arms[name]) for name in args.arms.split(",")]
print(f"{S} streams x {NW} windows per tick, {T} ticks per arm, {args.rounds} rounds; us per tick: p50 / mean / p95")
want = None
for name, arm in arms:                     # warm-up: first launches load the code objects
    out, _ = arm()
    want = out if want is None else want
    assert np.array_equal(out, want), f"{name}: probabilities differ from {arms[0][0]}"
print(f"all arms give the same {want.size} probabilities bit for bit (mean {want.mean():.4f}, max {want.max():.4f})")
for r in range(args.rounds):
    parts = []
    for name, arm in arms:
        _, us = arm()
        parts.append(f"{name} {np.median(us):.1f} / {us.mean():.1f} / {np.percentile(us, 95):.1f}")
    print(f"round {r}: " + " | ".join(parts), flush=True)
lib.wlk_vad_destroy(wh)
