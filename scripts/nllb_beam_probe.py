#!/usr/bin/env python
"""NLLB beam search: the host path against device beam steps, NLLB-200-distilled-600M shape, seeded weights
(GPU only).

    python scripts/nllb_beam_probe.py > profiles/nllb_beam_steps_mi355x.txt

(a) `nllb.beam_search(device_steps=False)`: top-k on the device for 2 n <= 8, the rows' logits read back and cut in numpy
    for 5 .. 8 beams, `kv_reorder` (a gather of the whole self-attention cache) after every step;
(b) `nllb.beam_search(device_steps=True)`: one `step_beam` graph replay per token, top-2n on the device for every n.
One 24-token source, up to 48 generated tokens, beams 2, 4, 5, 8; the two paths alternate for ROUNDS rounds after a warm-up of
both on the same session.  The figure is ms per generated token POSITION - per decoder step of the search (every beam row
advances one token), counted on the session - median (best) over the rounds: with seeded weights the answer may be a
hypothesis that ended after a few tokens while the search ran on to its stopping rule, so the answer's length is no
measure of the work.  The sequences of the two paths are compared.
(c) the two top-k forms alone through `wlk_diag_topk` (upload, two launches, read-back; the launches are the same ones a
    step uses) at V = 256 206, 8 rows, k = 8: form 0 = the existing kernel, form 1 = the wide one, alternating, enough
    repetitions to fill about half a second per form.  The upload and the read-back are the same for both forms, so the
    difference of the two figures is the difference of the kernels.
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SRC_LEN, MAX_NEW, ROUNDS = 24, 48, 3


class Counted:
    """The session with its decoder steps counted (the prompt and every single-token step, whichever call makes it)."""
    def __init__(self, sess):
        self._s, self.steps = sess, 0

    def __getattr__(self, name):
        attr = getattr(self._s, name)
        if name not in ("decode", "step", "step_beam"):
            return attr

        def counted(*a, **kw):
            self.steps += 1
            return attr(*a, **kw)
        return counted


def main():
    from whisperlivekit_amd import _lib, nllb
    if _lib.device_count() < 1:
        raise SystemExit("nllb_beam_probe: no HIP device (there is nothing to measure without one)")
    cfg = nllb.NLLB_200_DISTILLED_600M
    model = nllb.HipNllbModel.from_hf_state_dict(cfg, nllb.synth_state_dict(cfg, 1), device=0, max_src=64, max_tgt=64)
    rng = np.random.default_rng(3)
    src = np.concatenate([[256047], rng.integers(4, 250000, size=SRC_LEN - 2), [2]]).astype(np.int64)
    print(f"# NLLB-200-distilled-600M shape, seeded weights (synth_state_dict(cfg, 1)), fp32; source {SRC_LEN} tokens, "
          f"max_new_tokens {MAX_NEW}; ms per generated token position (= decoder step of the search), median (best) of {ROUNDS} "
          "rounds, host path and device steps alternating on one session after a warm-up of both")
    rows = []
    for n in (2, 4, 5, 8):
        sess = Counted(model.new_session(n))
        kw = dict(num_beams=n, max_new_tokens=MAX_NEW)
        for dev in (False, True):                                              # code objects, graph recordings
            nllb.beam_search(sess, src, 256057, device_steps=dev, **kw)
        t = {False: [], True: []}
        out, steps = {}, {}
        for _ in range(ROUNDS):
            for dev in (False, True):
                sess.steps = 0
                a = time.perf_counter()
                out[dev] = nllb.beam_search(sess, src, 256057, device_steps=dev, **kw)
                t[dev].append(time.perf_counter() - a)
                steps[dev] = sess.steps
        ms = lambda v, d: round(1e3 * v / steps[d], 3)
        r = dict(beams=n, steps_host=steps[False], steps_device=steps[True], answer_tokens=len(out[True]) - 1,
                 identical=out[False] == out[True],
                 host_ms_per_token=ms(statistics.median(t[False]), False), host_best=ms(min(t[False]), False),
                 device_ms_per_token=ms(statistics.median(t[True]), True), device_best=ms(min(t[True]), True),
                 ancestry_steps=sess.beam_stats()["ancestry_steps"])
        r["host_over_device"] = round(r["host_ms_per_token"] / r["device_ms_per_token"], 2)
        rows.append(r)
        print(json.dumps(r))
        sess.close()
    print("| beams | steps | (a) host path ms/token | (b) device steps ms/token | (a)/(b) | same ids |")
    print("|---:|---:|---:|---:|---:|---:|")
    for r in rows:
        print(f"| {r['beams']} | {r['steps_device']} | {r['host_ms_per_token']} ({r['host_best']}) | "
              f"{r['device_ms_per_token']} ({r['device_best']}) | {r['host_over_device']} | {r['identical']} |")
    model.close()

    # (c) the two top-k forms alone
    lib = _lib.load()
    V, R, k = 256206, 8, 8
    x = (np.random.default_rng(0).standard_normal((R, V)) * 3).astype(np.float32)
    vals = {f: np.empty((R, k), np.float32) for f in (0, 1)}
    ids = {f: np.empty((R, k), np.int32) for f in (0, 1)}

    def call(form):
        rc = lib.wlk_diag_topk(x.ctypes.data_as(C.c_void_p), R, V, k, form, vals[form].ctypes.data_as(C.c_void_p),
                               ids[form].ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise SystemExit(f"wlk_diag_topk form {form}: {rc} {lib.wlk_diag_last_error()}")

    for f in (0, 1, 0, 1):
        call(f)
    a = time.perf_counter()
    call(0)
    reps = max(5, int(0.5 / max(time.perf_counter() - a, 1e-6)))
    per = {0: [], 1: []}
    for _ in range(reps):
        for f in (0, 1):
            a = time.perf_counter()
            call(f)
            per[f].append(1e6 * (time.perf_counter() - a))
    same = bool(np.array_equal(vals[0].view(np.uint32), vals[1].view(np.uint32)) and np.array_equal(ids[0], ids[1]))
    print(json.dumps(dict(topk_alone=dict(n_vocab=V, rows=R, k=k, repetitions=reps, form0_us_median=round(statistics.median(per[0]), 1),
                                          form0_us_best=round(min(per[0]), 1), form1_us_median=round(statistics.median(per[1]), 1),
                                          form1_us_best=round(min(per[1]), 1),
                                          form0_minus_form1_us=round(statistics.median(per[0]) - statistics.median(per[1]), 1),
                                          bitwise_equal=same))))


if __name__ == "__main__":
    main()
