#!/usr/bin/env python
"""CIF end-of-word head on the device: what the host path costs a streaming call, what the device path costs,
and what the two kernels take.  base.en and large-v3 shapes, seeded weights, a seeded head (GPU only; one process, one box).

    python scripts/cif_probe.py > profiles/cif_device_mi355x.txt

Per model: one 30 s stream of seeded speech-like audio in 1 s chunks through HipSimulStreamingOnlineProcessor, three ways -
CIF off (no checkpoint: always fire), the host path (`cif_ckpt_path`, read-back + torch on the CPU) and the device path
(`cif_device=True`) - alternating, ROUNDS rounds after a warm-up round of each; wall time of insert_audio_chunk +
process_iter per call, mean over the stream's calls, median (best) over the rounds.  CIF off decodes another token stream
(it always fires), so the host and the device column are compared with each other first and with "off" second.  Inside the
calls: the wall time of the fire_at_boundary hook (host path: export + torch) and of the record read after the decode
loop (device path).  Then the two kernels' times from wlk_prof_* over encodes of the full 30 s buffer (T = 1500).
"""
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("WLK_SYNTHETIC_VOCAB", "1")   # seeded random weights: the stand-in vocabulary

SECONDS, CHUNK, ROUNDS = 30.0, 16000, 5


def seeded_head(d, path):
    import torch
    rng = np.random.default_rng(7000 + d)
    w = (0.25 * np.sqrt(128.0 / d) * rng.standard_normal(d)).astype(np.float32)
    torch.save({"weight": torch.from_numpy(w).reshape(1, d), "bias": torch.tensor([-1.0])}, path)
    return w


def run_stream(asr, audio):
    from whisperlivekit_amd.backend import HipSimulStreamingOnlineProcessor
    proc = HipSimulStreamingOnlineProcessor(asr)
    hook = {"t": 0.0, "read": 0.0, "fires": []}
    fire0 = proc.model.fire_at_boundary

    class Timed:                        # times the deferred read of the device path's answer
        def __init__(self, inner):
            self.inner = inner

        def __bool__(self):
            a = time.perf_counter()
            r = bool(self.inner)
            hook["read"] += time.perf_counter() - a
            return r

    def _fire(feature):
        a = time.perf_counter()
        r = fire0(feature)
        hook["t"] += time.perf_counter() - a
        r = r if isinstance(r, bool) else Timed(r)
        hook["fires"].append(r)
        return r

    proc.model.fire_at_boundary = _fire
    per_call, t_end, words = [], 0.0, 0
    try:
        for lo in range(0, len(audio), CHUNK):
            t_end += len(audio[lo:lo + CHUNK]) / 16000
            a = time.perf_counter()
            proc.insert_audio_chunk(audio[lo:lo + CHUNK].copy(), t_end)
            toks, _ = proc.process_iter()
            per_call.append(time.perf_counter() - a)
            if getattr(proc, "last_error", None) is not None:
                raise proc.last_error
            words += len(toks)
        exports = proc.model.session.export_calls.get("enc", 0)
        return dict(ms=1e3 * statistics.mean(per_call), hook_us=1e6 * hook["t"] / len(per_call),
                    read_us=1e6 * hook["read"] / len(per_call), fires=[bool(f) for f in hook["fires"]], words=words,
                    exports=exports, calls=len(per_call))
    finally:
        proc.close()


def kernel_times(model, audio, w):
    model.set_cif(w, -1.0)
    s = model.new_session(batched=False)
    try:
        s.append(audio)
        s.encode()
        s.cif_result()
        s.prof_begin()
        for _ in range(5):
            s.encode()
        s.sync()
        prof = s.prof_end(cap=128)
        total = sum(v["ms"] for v in prof.values())
        return {k: 1e3 * prof[k]["ms"] / prof[k]["launches"] for k in ("cif_alpha", "cif_decide")}, 1e3 * total / 5
    finally:
        s.close()
        model.set_cif(None)


def main():
    from whisperlivekit_amd import _lib, synth
    from whisperlivekit_amd.backend import HipSimulStreamingASR
    from whisperlivekit_amd.engine import HipWhisperModel
    if _lib.device_count() < 1:
        raise SystemExit("cif_probe: no HIP device (there is nothing to measure without one)")
    audio = synth.to_pcm16_roundtrip(synth.speech_like(SECONDS, 0))
    tmp = tempfile.mkdtemp(prefix="cif_probe_")
    print(f"# CIF head: host path vs device path; {SECONDS:.0f} s stream, {CHUNK / 16000:.1f} s chunks, seeded weights and head, "
          f"{ROUNDS} alternating rounds, median (best)")
    for name in ("base.en", "large-v3"):
        print(f"[{name}] seeded weights ...", file=sys.stderr, flush=True)
        model = HipWhisperModel.synthetic(name, 0)
        d = model.dims.n_audio_state
        ckpt = os.path.join(tmp, f"cif_{d}.pt")
        w = seeded_head(d, ckpt)
        kw = dict(hip_model=model)
        modes = {"off": dict(), "host": dict(cif_ckpt_path=ckpt, cif_device=False),
                 "device": dict(cif_ckpt_path=ckpt, cif_device=True)}

        def one(mode):
            asr = HipSimulStreamingASR(name, **kw, **modes[mode])
            try:
                return run_stream(asr, audio)
            finally:
                if mode == "device":            # the head belongs to the shared model: take it off again for the other modes
                    model.set_cif(None)
                    model._cif_path = None
                    model.cif_device = False

        res = {m: [] for m in modes}
        for m in modes:
            one(m)                              # warm-up: code objects, graph recordings
        for i in range(ROUNDS):
            for m in modes:
                res[m].append(one(m))
            print(f"[{name}] round {i + 1} of {ROUNDS}", file=sys.stderr, flush=True)
        med = lambda m, k: statistics.median(r[k] for r in res[m])
        best = lambda m, k: min(r[k] for r in res[m])
        print(f"\n## {name} (d = {d}; read-back of the host path: {1500 * d * 4 / 1e6:.2f} MB per call"
              f"{', after an X3 unpack kernel' if d >= 1024 else ''})")
        print("| path | ms per call | vs CIF off, ms | hook us per call | deferred read us per call | export(\"enc\") calls | words |")
        print("|---|---:|---:|---:|---:|---:|---:|")
        for m in modes:
            print(f"| {m} | {med(m, 'ms'):.3f} ({best(m, 'ms'):.3f}) | {med(m, 'ms') - med('off', 'ms'):+.3f} | "
                  f"{med(m, 'hook_us'):.1f} ({best(m, 'hook_us'):.1f}) | {med(m, 'read_us'):.1f} | {res[m][-1]['exports']} | "
                  f"{res[m][-1]['words']} |")
        same = all(r["fires"] == res["host"][0]["fires"] for r in res["host"] + res["device"])
        print(f"host minus device: {med('host', 'ms') - med('device', 'ms'):+.3f} ms per call (median of rounds; "
              f"{res['host'][0]['calls']} calls per stream); the two paths' fire sequences are "
              f"{'identical' if same else 'NOT identical (a case below the margin: the streams decode different tokens)'}; "
              f"fires {sum(res['host'][0]['fires'])} of {len(res['host'][0]['fires'])}")
        k, enc_us = kernel_times(model, audio, w)
        print(f"kernels at T = 1500 (wlk_prof_*, mean of 5 encodes): cif_alpha {k['cif_alpha']:.1f} us, cif_decide "
              f"{k['cif_decide']:.1f} us; the whole encode chain {enc_us:.0f} us")
        model.close()


if __name__ == "__main__":
    main()
