"""float64 restatement of the reference's CIF end-of-word test (simul_whisper/eow_detection.py:37-77) for the device
CIF tests, the seeded inputs of tests/golden/cif_device_kat.npz, and the rule that says when a case is *decided*.

The decision is discrete: a rounding, threshold tests inside ``resize``, a floor and two comparisons of the integral
against an integer.  An fp32 evaluation in another summation order (the device kernels) can land on the other side of
any of them when the float64 operands are closer than fp32 rounding.  A case is decided when every such comparison
has ``|lhs - rhs| > R * max(1, |rhs|)``; R is 100x the largest relative deviation of the reference's own fp32
``integrate`` from this float64 evaluation, measured by scripts/gen_golden_cif_device.py and stored in the fixture.
"""
import numpy as np

THRESHOLD = 0.999
KINDS = ("noise", "boundary", "quiet_tail", "peaks")
T_VALUES = (2, 3, 4, 5, 8, 13, 25, 50, 63, 64, 65, 127, 128, 129, 255, 256, 257, 400, 901, 1499, 1500)
SCALES = (0.25, 1.0, 2.0)
D_VALUES = (128, 384, 1280)


def make_head(d):
    """The fixture's seeded head for width d: w ~ 0.25 N(0, 1) * sqrt(128 / d), b = -1.  The factor keeps the spread of
    the pre-activation x.w at every width what cif_kat.json's d = 128 head has (std 2.8 at scale 1).  Without it the
    d = 1280 head sees pre-activations of std 9 at scale 1, nearly every alpha saturates, and the reference's own fp32
    error (6e-7 .. 1.2e-6 over five seed bases) puts R at 6e-5 or more and 35-47 % of the cases below the margin."""
    rng = np.random.default_rng(7000 + d)
    return (0.25 * np.sqrt(128.0 / d) * rng.standard_normal(d)).astype(np.float32), -1.0


def make_features(seed, T, d, kind, scale, w):
    """fp32 [T, d] features of one fixture case (u = w / (w.w): adding c*u moves the head's pre-activation by c)."""
    rng = np.random.default_rng(int(seed))
    x = rng.standard_normal((int(T), int(d)), dtype=np.float32) * np.float32(scale)
    u = (w.astype(np.float64) / float(np.dot(w.astype(np.float64), w.astype(np.float64)))).astype(np.float32)
    if kind == "boundary":
        x[T - 2] += np.float32(8.0) * u
    elif kind == "quiet_tail":
        x[max(T - 5, 0):] -= np.float32(6.0) * u
    elif kind == "peaks":
        x[::7] += np.float32(9.0) * u
    elif kind != "noise":
        raise ValueError(kind)
    return np.ascontiguousarray(x, dtype=np.float32)


def alphas64(x, w, bias):
    z = x.astype(np.float64) @ w.astype(np.float64) + float(bias)
    return 1.0 / (1.0 + np.exp(-z))


def alpha_bound(x, w):
    """Per-row bound on |alpha_fp32 - alpha_float64| for ANY fp32 summation order of the dot product:
    0.25 (sigmoid's largest slope) * d * 2^-24 * sum_i |x_i w_i|  (worst-case rounding of a d-term fp32 dot product)
    + 4 * 2^-24 (the bias add, exp, the add and the divide of the sigmoid itself)."""
    d = x.shape[1]
    s = np.abs(x.astype(np.float64) * w.astype(np.float64)[None, :]).sum(axis=1)
    return 0.25 * d * 2.0 ** -24 * s + 4 * 2.0 ** -24


class _Margins:
    def __init__(self, R):
        self.R, self.decided, self.why = float(R), True, None

    def fail(self, what):
        if self.decided:
            self.why = what
        self.decided = False

    def check(self, lhs, rhs, what):
        if not (abs(lhs - rhs) > self.R * max(1.0, abs(rhs))):     # NaN counts as undecided
            self.fail(what)


def evaluate(x, w, bias, R):
    """-> dict(fire, decided, why, n, cnt, pos, resize_rounds, updates, total, integ (float64 [T-1]), alpha (float64 [T]))
    for features x [T, d] (T >= 2)."""
    T = x.shape[0]
    if T < 2:
        raise IndexError("index -1 is out of bounds for dimension 0 with size 0")
    alpha = alphas64(x, w, bias)
    return evaluate_alphas(alpha, R)


def evaluate_alphas(alpha, R):
    alpha = np.asarray(alpha, dtype=np.float64)
    T = alpha.shape[0]
    mg = _Margins(R)
    total = float(alpha.sum())
    n = float(np.rint(total))                                  # ties to even, as torch.round
    mg.check(total, np.floor(total) + 0.5, "round")
    a = alpha * (n / total) if total != 0 else alpha * np.nan
    rounds = updates = 0
    while True:
        over = a > THRESHOLD
        # every element's threshold test of this round's snapshot (the loop condition is their disjunction)
        if not (np.abs(a - THRESHOLD) > mg.R * 1.0).all():          # (max(1, 0.999) = 1; NaN counts as undecided)
            mg.fail("resize snapshot")
        if not over.any():
            break
        rounds += 1
        if rounds > 10:
            rounds = 10
            break
        for idx in np.nonzero(over)[0]:
            mg.check(float(a[idx]), THRESHOLD, "resize visit")
            if a[idx] >= THRESHOLD:
                mask = (a != 0).astype(np.float64)
                a = a * 0.5 + (0.5 * a.sum() / mask.sum()) * mask
                updates += 1
    integ = np.cumsum(a[:-1])
    last = float(integ[-1])
    k = np.rint(last / THRESHOLD)
    mg.check(last, k * THRESHOLD, "floor")
    cnt = float(np.floor(last / THRESHOLD))
    mg.check(float(integ[T - 2]), cnt, "integ[T-2] vs cnt")
    if T >= 3:
        mg.check(float(integ[T - 3]), cnt, "integ[T-3] vs cnt")
    r = integ - cnt
    hits = np.nonzero(r >= 0)[0]
    pos = int(hits[0]) if hits.size else -1
    fire = bool(hits.size and pos >= T - 2)
    return dict(fire=fire, decided=mg.decided, why=mg.why, n=int(n) if np.isfinite(n) else -1,
                cnt=int(cnt) if np.isfinite(cnt) else -1, pos=pos, resize_rounds=rounds, updates=updates, total=total,
                integ=integ, alpha=alpha)


def no_resize_cross_check(ev, T):
    """Without the resize loop the answer equals integ[T-3] < cnt <= integ[T-2] (integ is monotone)."""
    integ, cnt = ev["integ"], ev["cnt"]
    if T == 2:                                                 # one element: pos = 0 iff integ[0] >= cnt
        return bool(cnt <= integ[0])
    return bool(integ[T - 3] < cnt <= integ[T - 2])


_FIXTURE_CACHE = {}


def load_fixture(path):
    """-> dict(R, max_rel_dev, heads {d: (w, b)}, cases [dict(d, seed, T, kind, scale, fire)])"""
    if path in _FIXTURE_CACHE:
        return _FIXTURE_CACHE[path]
    z = np.load(path)
    heads = {int(d): (z[f"w_{int(d)}"].astype(np.float32), float(z["bias"])) for d in z["d_values"]}
    cases = [dict(d=int(d), seed=int(s), T=int(t), kind=KINDS[int(k)], scale=float(sc), fire=bool(f))
             for d, s, t, k, sc, f in zip(z["case_d"], z["case_seed"], z["case_T"], z["case_kind"], z["case_scale"],
                                          z["case_fire"])]
    out = dict(R=float(z["R"]), max_rel_dev=float(z["max_rel_dev"]), heads=heads, cases=cases)
    _FIXTURE_CACHE[path] = out
    return out


_EVAL_CACHE = {}


def iter_fixture(path):
    """Yields (case, x fp32 [T, d], float64 evaluation) for every case.  Features are not stored: they are regenerated
    from the seed on every pass; the evaluations are computed once per process and shared."""
    fx = load_fixture(path)
    evs = _EVAL_CACHE.setdefault(path, {})
    for i, c in enumerate(fx["cases"]):
        w, b = fx["heads"][c["d"]]
        x = make_features(c["seed"], c["T"], c["d"], c["kind"], c["scale"], w)
        if i not in evs:
            evs[i] = evaluate(x, w, b, fx["R"])
        yield c, x, evs[i]


def kat_features(k):
    """The features of one tests/golden/cif_kat.json case, as scripts/gen_golden.py:gen_cif draws them."""
    import torch
    return (torch.randn(1, k["T"], 128, generator=torch.Generator().manual_seed(k["seed"])) * k["scale"])[0].numpy()
