#!/usr/bin/env python
"""Every NLLB entry point that enqueues the encoder or the decoder layer chain, once, on the micro shape with seeded
weights (GPU only) - what a change to the composition of those chains is compared on, tree against tree:

    python scripts/nllb_chain_probe.py [--out DIR]          run; with --out every result below is stored as DIR/<name>.npy
    rocprofv3 --kernel-trace --stats --output-format csv -d D -o t -- python scripts/nllb_chain_probe.py
                                                            the same run under the profiler (no other tracing, one run per tree)
    python scripts/nllb_chain_probe.py --compare-out A B [C]  largest |A - B| per array; with C also |A - C| (A, C: two runs of
                                                            one tree, B: the other tree)
    python scripts/nllb_chain_probe.py --compare-trace A.csv B.csv   two *_kernel_trace.csv: calls per kernel name side by
                                                            side, and whether the names come in the same order

Session, 3 rows: encode, decode(first=1) of a 3-token prompt, two step, set_alignment_heads, two step_align, two step_beam
with k = 12.  Batch, 3 slots: encode of lengths 5 / 7 / 9, prefill of 2-token prompts, two step of 3 rows, one step of 1 row,
two step_align.  Stored: every logits() / logits(slot), every top-k pair, every alignment() export, every encoder_output.
"""
import csv
import glob
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HEADS = [(0, 1), (1, 0)]


def run(out_dir):
    from whisperlivekit_amd import _lib, nllb
    if _lib.device_count() < 1:
        raise SystemExit("nllb_chain_probe: no HIP device (there is nothing to run without one)")
    kept = {}

    def keep(name, *arrays):
        for i, a in enumerate(arrays):
            kept[f"{name}.{i}"] = np.array(a, copy=True)

    cfg = nllb.NLLB_MICRO
    model = nllb.HipNllbModel.synthetic(cfg, seed=1, device=0, max_src=32, max_tgt=32)
    rng = np.random.default_rng(5)

    def sentence(n):
        return np.concatenate([[7], rng.integers(4, cfg.vocab_size, size=n - 2), [2]]).astype(np.int64)

    rows = 3
    sess = model.new_session(rows)
    sess.encode(sentence(7))
    keep("s.enc", sess.encoder_output())
    sess.decode(np.array([[2, 9, 11 + r] for r in range(rows)]), first=True)
    keep("s.decode.logits", sess.logits())
    keep("s.decode.topk", *sess.topk(4))
    ids = np.array([20, 21, 22])
    for i in range(2):
        lp, ids2 = sess.step(ids, 4)
        keep(f"s.step{i}", lp, ids2, sess.logits())
        ids = ids2[:, 0]
    sess.set_alignment_heads(HEADS)
    for i in range(2):
        out = sess.step_align(ids, 4, 1, 6, 5)
        keep(f"s.align{i}", *out, sess.logits(), sess.alignment())
        ids = out[1][:, 0]
    for i, src in enumerate(([0, 0, 1], [2, 0, 0])):
        lp, ids2 = sess.step_beam(ids, src, 12)
        keep(f"s.beam{i}", lp, ids2, sess.logits())
        ids = ids2[:, i]
    sess.close()

    slots = [0, 1, 2]
    batch = model.new_batch(3)
    batch.encode(slots, [sentence(n) for n in (5, 7, 9)])
    for s in slots:
        keep(f"b.enc{s}", batch.encoder_output(s))
    batch.prefill(slots, [[2, 30 + s] for s in slots])
    ids = np.array([40, 41, 42])
    for i in range(2):
        lp, ids2 = batch.step(slots, ids, 4)
        keep(f"b.step{i}", lp, ids2, *[batch.logits(s) for s in slots])
        ids = ids2[:, 0]
    lp, ids1 = batch.step([1], ids[1:2], 4)
    keep("b.step_one", lp, ids1, batch.logits(1))
    ids[1] = ids1[0, 0]
    batch.set_alignment_heads(HEADS)
    for i in range(2):
        out = batch.step_align(slots, ids, 4, [1, 1, 1], [4, 6, 8], [3, 5, 7])
        keep(f"b.align{i}", *out, *[batch.logits(s) for s in slots], *[batch.alignment(s) for s in slots])
        ids = out[1][:, 0]
    batch.close()
    model.close()
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        for name, a in kept.items():
            np.save(os.path.join(out_dir, name + ".npy"), a)
    print(f"nllb_chain_probe: {len(kept)} arrays" + (f" stored under {out_dir}" if out_dir else ""))


def load(d):
    return {os.path.basename(p)[:-4]: np.load(p) for p in sorted(glob.glob(os.path.join(d, "*.npy")))}


def largest(a, b):
    if a.shape != b.shape:
        return float("inf")
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()) if a.size else 0.0


def compare_out(a_dir, b_dir, c_dir=None):
    a, b = load(a_dir), load(b_dir)
    c = load(c_dir) if c_dir else None
    if set(a) != set(b) or (c is not None and set(a) != set(c)):
        raise SystemExit("nllb_chain_probe: the runs did not store the same arrays")
    worst_b = worst_c = 0.0
    equal_b = equal_c = True
    for name in sorted(a):
        worst_b = max(worst_b, largest(a[name], b[name]))
        equal_b = equal_b and np.array_equal(a[name], b[name])
        if c is not None:
            worst_c = max(worst_c, largest(a[name], c[name]))
            equal_c = equal_c and np.array_equal(a[name], c[name])
    print(f"{len(a)} arrays, {sum(v.size for v in a.values())} values")
    if c is not None:
        print(f"{a_dir} against {c_dir}: array_equal {equal_c}, largest difference {worst_c:g}")
    print(f"{a_dir} against {b_dir}: array_equal {equal_b}, largest difference {worst_b:g}")
    return 0 if (equal_b if (c is None or equal_c) else worst_b <= worst_c) else 1


def kernel_names(path):
    with open(path, newline="") as fh:
        rows = list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return [r["Kernel_Name"] for r in rows]


def compare_trace(a_csv, b_csv):
    a, b = kernel_names(a_csv), kernel_names(b_csv)
    count = lambda names: {n: names.count(n) for n in dict.fromkeys(names)}
    ca, cb = count(a), count(b)
    print(f"{'kernel':<72}{'parent':>8}{'new':>8}")
    for n in sorted(set(ca) | set(cb), key=lambda n: (-ca.get(n, 0), n)):
        print(f"{n[:70]:<72}{ca.get(n, 0):>8}{cb.get(n, 0):>8}")
    print(f"{'all kernels':<72}{len(a):>8}{len(b):>8}")
    print(f"# per-name counts equal: {ca == cb}; the two traces are the same kernel names in the same order: {a == b}")
    return 0 if a == b else 1


if __name__ == "__main__":
    if "--compare-out" in sys.argv:
        sys.exit(compare_out(*sys.argv[sys.argv.index("--compare-out") + 1:][:3]))
    if "--compare-trace" in sys.argv:
        i = sys.argv.index("--compare-trace")
        sys.exit(compare_trace(sys.argv[i + 1], sys.argv[i + 2]))
    run(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None)
