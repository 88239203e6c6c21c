#!/usr/bin/env python
"""Generate tests/golden/cif_device_kat.npz: known answers of the UNMODIFIED reference's fire_at_boundary
(simul_whisper/eow_detection.py:62-77, on CPU) for the device CIF head's tests.

For d in {128, 384, 1280}: one seeded head (tests/cif_reference.py:make_head) and, for every T of T_VALUES x kind of KINDS
x scale of SCALES, the generator seed and the reference's boolean.  Features are regenerated from the seed by the tests
(cif_reference.make_features), not stored.  Also measured and stored: the largest relative deviation of the reference's
own fp32 `integrate` from the float64 restatement (cif_reference.evaluate), and R = 100x that, rounded up to one digit -
the margin below which a case counts as undecided.  The conditions the tests rely on are asserted here.

Run where the reference is importable (the stubs of scripts/ref_stubs.py):  python scripts/gen_golden_cif_device.py
"""
import json
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import ref_stubs  # noqa: E402

ref_stubs.install()

from whisperlivekit.simul_whisper.eow_detection import fire_at_boundary, resize  # noqa: E402

import cif_reference as cr  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")
torch.set_num_threads(8)


def linear(w, b):
    lin = torch.nn.Linear(w.size, 1)
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(w).reshape(1, -1))
        lin.bias.copy_(torch.tensor([float(b)]))
    return lin


def reference_integrate(x, lin):
    """The reference's fp32 `integrate` (before the subtraction) and n, from its own resize() and operators."""
    with torch.no_grad():
        alphas = torch.sigmoid(lin(torch.from_numpy(x).unsqueeze(0)).squeeze(dim=2))
        n = torch.round(alphas.sum(-1)).int()
        a, _ = resize(alphas, n)
        return torch.cumsum(a.squeeze(0)[:-1], dim=0).double().numpy(), int(n[0])


def main():
    heads = {d: cr.make_head(d) for d in cr.D_VALUES}
    cases = []
    seed = 20000
    for d in cr.D_VALUES:
        w, b = heads[d]
        lin = linear(w, b)
        for T in cr.T_VALUES:
            for ki, kind in enumerate(cr.KINDS):
                for scale in cr.SCALES:
                    seed += 1
                    x = cr.make_features(seed, T, d, kind, scale, w)
                    with torch.no_grad():
                        fire = bool(fire_at_boundary(torch.from_numpy(x).unsqueeze(0), lin))
                    integ32, n32 = reference_integrate(x, lin)
                    cases.append(dict(d=d, seed=seed, T=T, kind=ki, scale=scale, fire=fire, integ32=integ32, n32=n32))
    # the reference's own fp32 error: relative deviation of its integrate from float64, over the cases where both take
    # the same path through the discrete steps before it (same n, same number of resize updates - checked through the
    # values themselves: a different path moves integrate by far more than rounding, so those cases are left out by a
    # coarse 1e-3 screen and counted)
    max_dev, screened = 0.0, 0
    for c in cases:
        w, b = heads[c["d"]]
        x = cr.make_features(c["seed"], c["T"], c["d"], cr.KINDS[c["kind"]], c["scale"], w)
        ev = cr.evaluate(x, w, b, 0.0)
        dev = np.abs(c["integ32"] - ev["integ"]) / np.maximum(1.0, np.abs(ev["integ"]))
        worst = float(np.nanmax(dev)) if dev.size else 0.0
        if c["n32"] != ev["n"] or not (worst < 1e-3):
            screened += 1
            continue
        max_dev = max(max_dev, worst)
    exp = math.floor(math.log10(100 * max_dev))
    R = math.ceil(100 * max_dev / 10 ** exp) * 10 ** exp
    print(f"reference fp32 integrate vs float64: max relative deviation {max_dev:.3e} over {len(cases) - screened} cases "
          f"({screened} on another discrete path), R = {R:.1e}")

    # the conditions the tests rely on
    stats = {}
    resize_cases = 0
    for c in cases:
        w, b = heads[c["d"]]
        x = cr.make_features(c["seed"], c["T"], c["d"], cr.KINDS[c["kind"]], c["scale"], w)
        ev = cr.evaluate(x, w, b, R)
        st = stats.setdefault(c["d"], dict(n=0, undecided=0, fire=0, hold=0, mismatch=0))
        st["n"] += 1
        resize_cases += ev["resize_rounds"] > 0
        if not ev["decided"]:
            st["undecided"] += 1
            continue
        st["fire" if ev["fire"] else "hold"] += 1
        st["mismatch"] += ev["fire"] != c["fire"]
    for d, st in stats.items():
        print(d, st)
        assert 3 * st["undecided"] <= st["n"], f"d={d}: more than a third of the cases are undecided"
        assert st["mismatch"] == 0, f"d={d}: float64 disagrees with the reference on a decided case"
    assert sum(st["fire"] for st in stats.values()) >= 8 and sum(st["hold"] for st in stats.values()) >= 8
    assert resize_cases >= 20, resize_cases
    print("cases entering the resize loop:", resize_cases)

    kat = json.load(open(os.path.join(OUT, "cif_kat.json")))
    ck = torch.load(os.path.join(OUT, "cif_micro.pt"), map_location="cpu", weights_only=True)
    wk, bk = ck["weight"].float().numpy().reshape(-1), float(ck["bias"].reshape(-1)[0])
    und = fires = 0
    for k in kat:
        ev = cr.evaluate(cr.kat_features(k), wk, bk, R)
        und += not ev["decided"]
        fires += ev["decided"] and ev["fire"]
        assert not ev["decided"] or ev["fire"] == k["fire"], k
    print(f"cif_kat.json: {und} of {len(kat)} undecided, {fires} decided cases fire")

    np.savez_compressed(
        os.path.join(OUT, "cif_device_kat.npz"), R=np.float64(R), max_rel_dev=np.float64(max_dev),
        d_values=np.asarray(cr.D_VALUES, np.int32), bias=np.float64(-1.0),
        **{f"w_{d}": heads[d][0] for d in cr.D_VALUES},
        case_d=np.asarray([c["d"] for c in cases], np.int32), case_seed=np.asarray([c["seed"] for c in cases], np.int64),
        case_T=np.asarray([c["T"] for c in cases], np.int32), case_kind=np.asarray([c["kind"] for c in cases], np.int8),
        case_scale=np.asarray([c["scale"] for c in cases], np.float64), case_fire=np.asarray([c["fire"] for c in cases], bool))
    print("wrote", os.path.join(OUT, "cif_device_kat.npz"))


if __name__ == "__main__":
    main()
