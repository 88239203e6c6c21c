"""Inputs of the token-selection / AlignAtt read-out tests: one generator module for test_select_reference_cpu.py (which
checks the references and the exclusion caps on these very cases) and test_gpu_select.py (which runs them on the device).

A case is a dict:
  name, kind ("random" | "planted" | "tie"), logits [R, V] f32, adj (rows, ids, deltas) or None, k, ns_token (-1 = none),
  ns_logits, ring [A, R, ring_rows, T] f32, counters (prefill_rows [R], n_single [R], newest_row [R], single_base),
  content_len [R], zero_cols (columns whose window is constant: z must be exactly 0 there).
Ring rows outside the window are NaN: a kernel that reads one poisons its output."""
import numpy as np

SLICES = 64                 # kSelBlocks of select.hip
NEG_INF = np.float32(-np.inf)


def slice_bounds(V, s):
    per = (V + SLICES - 1) // SLICES
    return s * per, min(V, (s + 1) * per)


# ------------------------------------------------------------------------------------------------------------------
# alignment windows
# ------------------------------------------------------------------------------------------------------------------
def _softmax_rows(rng, shape):
    s = 2.0 * rng.standard_normal(shape)
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def comb(p, T, high=6.0, mid=1.5):
    """a planted peak the width-7 median keeps: four high columns at p -3, -1, +1, +3 (only the window centred on p holds all
    four, counting the reflected ones at the ends), the columns between them at a lower level"""
    amps = {}
    for d, a in ((-3, high), (-1, high * 1.1), (1, high * 1.2), (3, high * 0.9), (-2, mid), (0, mid * 1.2), (2, mid * 0.8)):
        f = p + d
        if 0 <= f < T:
            amps[f] = a
    return amps


def make_ring(seed, A, B, T, windows, plants=None, period=None, const_cols=()):
    """windows: one (prefill_rows, n_single, newest_slot) for all beams or a list of B of them.  plants: {frame: amplitude}
    (or a list of B) - the newest row's column is set to the mean of the window's other rows + amplitude x their standard
    deviation.  period: columns repeat with this period (exact ties between frames).  const_cols: columns held constant
    over the whole window."""
    rng = np.random.default_rng(seed)
    if isinstance(windows, tuple):
        windows = [windows] * B
    if plants is None or isinstance(plants, dict):
        plants = [plants] * B
    pre_max = max(w[0] for w in windows)
    single_base = pre_max + 3
    ring_rows = single_base + 16
    ring = np.full((A, B, ring_rows, T), np.nan, np.float32)
    pre_l, ns_l, new_l = [], [], []
    for b, (pre, ns, slot) in enumerate(windows):
        rows = list(range(pre)) + [single_base + j for j in range(ns)]
        newest = single_base + slot if ns else pre - 1
        assert newest in rows
        T0 = period or T
        w = _softmax_rows(rng, (A, len(rows), T0))
        for c in const_cols:
            w[:, :, c] = 1.0 / T0
        if plants[b] and len(rows) > 1:
            ni = rows.index(newest)
            others = np.delete(w, ni, axis=1)
            for f, amp in plants[b].items():
                w[:, ni, f] = others[:, :, f].mean(axis=1) + amp * others[:, :, f].std(axis=1)
        if period:
            w = np.tile(w, (1, 1, (T + period - 1) // period))[:, :, :T] * (period / T)
        ring[:, b, rows, :] = w.astype(np.float32)
        pre_l.append(pre), ns_l.append(ns), new_l.append(newest)
    counters = (np.array(pre_l, np.int32), np.array(ns_l, np.int32), np.array(new_l, np.int32), single_base)
    return ring, counters


def _tiny_logits(seed, R):
    return (3.0 * np.random.default_rng(seed).standard_normal((R, 64))).astype(np.float32)


def _align_case(name, kind, seed, A, B, T, windows, content_len, plants=None, period=None, const_cols=()):
    def build():
        ring, counters = make_ring(seed, A, B, T, windows, plants, period, const_cols)
        cl = np.array(content_len if np.ndim(content_len) else [content_len] * B, np.int32)
        return dict(name=name, kind=kind, logits=_tiny_logits(seed + 1, B), adj=None, k=1, ns_token=-1, ns_logits=None,
                    ring=ring, counters=counters, content_len=cl, zero_cols=tuple(const_cols))
    return name, build


def _align_cases():
    T = 1500
    out = []
    add = lambda *a, **k: out.append(_align_case(*a, **k))
    # (prefill_rows, n_single) x heads x beams x content_len x peak position, walked diagonally
    add("win_1_0_a1b1", "tie", 100, 1, 1, T, (1, 0, 0), T, comb(700, T))          # one row: z = 0 everywhere, frame 0
    add("win_11_0_a2b1_peak0", "planted", 101, 2, 1, T, (11, 0, 0), 1499, comb(0, T))
    add("win_11_5_a6b3_peak1", "planted", 102, 6, 3, T, (11, 5, 4), 257, comb(1, T))
    add("win_11_15_a10b1_peak2", "planted", 103, 10, 1, T, (11, 15, 14), 256, comb(2, T))
    add("win_96_0_a5b7_peak3", "planted", 104, 5, 7, T, (96, 0, 0), 255, comb(3, T))
    add("win_97_3_a2b1_peakT1", "planted", 105, 2, 1, T, (97, 3, 2), T, comb(T - 1, T))
    add("win_200_15_a6b3_peakT2", "planted", 106, 6, 3, T, (200, 15, 14), T, comb(T - 2, T))
    add("win_447_1_a1b1_peakT3", "planted", 107, 1, 1, T, (447, 1, 0), T, comb(T - 3, T))
    add("win_11_5_a30b1_peakT4", "planted", 108, 30, 1, T, (11, 5, 4), T, comb(T - 4, T))   # beyond LDS: no fused form
    add("win_96_0_a2b1_mid", "planted", 109, 2, 1, T, (96, 0, 0), T, comb(1024, T))
    for slot in range(16):                                                       # prefill rows gone, every wrapped slot
        add(f"win_0_16_slot{slot}", "planted", 120 + slot, 2, 1, 257, (0, 16, slot), 257, comb(17 * slot % 250 + 3, 257))
    # content_len edges
    for cl in (0, 1):
        add(f"cl_{cl}", "planted", 140 + cl, 2, 2, T, (11, 5, 4), cl, comb(700, T))
    for cl in (3, 4):
        add(f"cl_{cl}", "planted", 140 + cl, 2, 2, T, (11, 5, 4), cl, {**comb(1, T), **comb(700, T, 9.0)})
    for cl in (255, 256, 257, 600, 1499):                                        # the highest peak sits AT content_len
        add(f"behind_cl_{cl}", "planted", 150 + cl, 2, 1, T, (11, 5, 4), cl, {**comb(cl - 40, T, 4.0, 1.0), **comb(cl + 3, T, 9.0, 5.0)})
        add(f"last_inside_cl_{cl}", "planted", 160 + cl, 2, 1, T, (11, 5, 4), cl, comb(cl - 1, T, 6.0, 0.5))
    # small T
    add("T257_peak255", "planted", 170, 2, 2, 257, (11, 5, 4), 257, comb(255, 257))
    add("T7", "planted", 171, 2, 1, 7, (11, 5, 4), 7, {0: 0.5, 1: 3.0, 2: 1.0, 3: 6.0, 4: 2.0, 5: 5.0, 6: 0.2})
    add("T4", "planted", 172, 2, 1, 4, (11, 5, 4), 4, {0: 0.5, 1: 5.0, 2: 3.0, 3: 1.0})
    add("T3", "planted", 173, 2, 1, 3, (11, 5, 4), 3, {0: 0.5, 1: 1.0, 2: 5.0})
    # exact ties: columns f and f + 250 are the same bits, so interior frames tie; the lowest one inside content_len wins
    add("tie_p100_a2b1", "tie", 180, 2, 1, T, (11, 5, 4), T, comb(100, 250), period=250)
    add("tie_p240_a6b3", "tie", 181, 6, 3, T, (11, 15, 3), T, comb(240, 250), period=250)
    add("tie_p100_cl360", "tie", 182, 5, 1, T, (96, 0, 0), 360, comb(100, 250), period=250)
    add("tie_p100_cl1000_a30", "tie", 183, 30, 1, T, (11, 5, 4), 1000, comb(100, 250), period=250)
    # a column that is constant over the window: std = 0, z = 0 / 1e-8
    add("const_col", "planted", 190, 2, 1, T, (11, 5, 4), T, comb(900, T), const_cols=(500, 0, T - 1))
    add("const_col_long", "planted", 191, 2, 1, T, (97, 3, 1), T, comb(900, T), const_cols=(64,))
    # per-row windows (batched engine form only): each row its own ring, counters and content_len
    add("rows4", "planted", 200, 2, 4, T, [(11, 0, 0), (11, 5, 4), (0, 16, 9), (97, 3, 2)], [0, 256, 1499, T],
        [comb(5, T), comb(255, T), comb(1400, T), comb(T - 1, T)])
    add("rows8", "planted", 201, 6, 8, T, [(1, 0, 0), (11, 5, 0), (11, 15, 7), (0, 16, 15), (96, 0, 0), (200, 15, 2), (447, 1, 0), (11, 1, 0)],
        [1, 3, 4, 255, 256, 257, 1499, T],
        [comb(0, T), comb(1, T), comb(2, T), comb(254, T), comb(255, T), comb(256, T), comb(1498, T), comb(T - 2, T)])
    return out


# ------------------------------------------------------------------------------------------------------------------
# logits
# ------------------------------------------------------------------------------------------------------------------
def _tiny_ring(seed, R):
    return make_ring(seed, 1, R, 64, (2, 1, 0), comb(20, 64))


def _topk_case(name, kind, seed, R, V, k, fill, with_adj=None, ns=None):
    def build():
        rng = np.random.default_rng(seed)
        x = (3.0 * rng.standard_normal((R, V))).astype(np.float32)
        if fill:
            fill(rng, x, k)
        adj = with_adj(rng, x, k) if with_adj else None
        ring, counters = _tiny_ring(seed + 7, R)
        ns_token, ns_logits = -1, None
        if ns is not None:
            ns_token = ns if ns >= 0 else V + ns
            ns_logits = (3.0 * rng.standard_normal((R, V))).astype(np.float32)
            ns_logits[0, (ns_token + 11) % V] = 80.0                       # one row with an outlier
            if R > 1:
                ns_logits[1, ns_token] = 9.0
        return dict(name=name, kind=kind, logits=x, adj=adj, k=k, ns_token=ns_token, ns_logits=ns_logits, ring=ring,
                    counters=counters, content_len=np.full(R, 64, np.int32), zero_cols=())
    return name, build


def _outliers(rng, x, k):
    V = x.shape[1]
    lo, hi = slice_bounds(V, 3)
    x[0, min(lo + 5, V - 1)] = 80.0
    if x.shape[0] > 1:
        x[1, V - 1] = 80.0                                                   # in the last (ragged) slice


def _all_equal(rng, x, k):
    x[:] = 1.5


def _few_finite(rng, x, k):
    """k - 1 finite logits per row, the rest -inf: rank k is the lowest-index -inf"""
    R, V = x.shape
    keep = x.copy()
    x[:] = NEG_INF
    for r in range(R):
        ids = rng.choice(V, k - 1, replace=False)
        if r == 1:
            ids[:2] = (0, 1)[:len(ids)]
        if r == 2:
            ids[0] = V - 1
        x[r, ids] = keep[r, ids]


def _tie_ids_across(V, n):
    """n indices in n different slices (the last one in the ragged last slice)"""
    last = (V - 1) // ((V + SLICES - 1) // SLICES)
    ids = []
    for j, s in enumerate([5, 17, 18, 40, 63, 0, 33, 62, 1, 2][:n]):
        lo, hi = slice_bounds(V, min(s, last))
        ids.append(lo + (j * 37) % (hi - lo))
    return sorted(set(ids))


def _ties_across(extra):
    def fill(rng, x, k):
        V = x.shape[1]
        for r in range(x.shape[0]):
            ids = _tie_ids_across(V, k + (extra if r else 0))
            x[r, ids] = 20.0
    return fill


def _ties_same_thread(rng, x, k):
    """ties inside one slice: indices 256 apart belong to one thread of the slice pass, the others to other waves"""
    V = x.shape[1]
    for r in range(x.shape[0]):
        lo, hi = slice_bounds(V, 9 + r)
        ids = [lo + 7 + 256 * j for j in range(8) if lo + 7 + 256 * j < hi][:4] + [lo + 100, lo + 199, lo + 70, lo + 250]
        x[r, ids[:k + r]] = 20.0


def _ties_slice_edges(rng, x, k):
    V = x.shape[1]
    last = (V - 1) // ((V + SLICES - 1) // SLICES)
    ids = []
    for s in (0, 7, 8, last):
        lo, hi = slice_bounds(V, s)
        ids += [lo, hi - 1]
    x[:, ids[:k + 1] if k < 8 else ids] = 20.0


def _adj_unique(n, mixed=False, boundaries=False):
    def make(rng, x, k):
        R, V = x.shape
        ids = set()
        if boundaries:
            for s in (0, 1, 31, 62, 63):
                lo, hi = slice_bounds(V, s)
                ids |= {lo, hi - 1}
        pool = rng.permutation(V)
        for i in pool:
            if len(ids) >= n:
                break
            ids.add(int(i))
        ids = rng.permutation(sorted(ids)[:n] if len(ids) > n else sorted(ids)).astype(np.int32)
        rows = (rng.integers(-1, R, len(ids)) if mixed else np.full(len(ids), -1)).astype(np.int32)
        deltas = (2.0 * rng.standard_normal(len(ids))).astype(np.float32)
        deltas[deltas == 0] = 1.0
        return rows, ids, deltas
    return make


def _adj_suppress(whole_slice):
    """-inf on the current top-k of every row (all rows), a DRY-style finite penalty on each row's next best (that row
    only), and optionally one whole slice suppressed"""
    def make(rng, x, k):
        R, V = x.shape
        order = np.argsort(-x, axis=1, kind="stable")
        top = sorted({int(i) for i in order[:, :k].ravel()})
        rows, ids, deltas = [-1] * len(top), list(top), [NEG_INF] * len(top)
        for r in range(R):
            nxt = next(int(i) for i in order[r] if int(i) not in top)
            rows.append(r), ids.append(nxt), deltas.append(np.float32(-2.5))
        if whole_slice:
            lo, hi = slice_bounds(V, 10)
            taken = set(ids)
            for i in range(lo, hi):
                if i not in taken:
                    rows.append(-1), ids.append(i), deltas.append(NEG_INF)
        return np.array(rows, np.int32), np.array(ids, np.int32), np.array(deltas, np.float32)
    return make


def _topk_cases():
    out = []
    add = lambda *a, **k: out.append(_topk_case(*a, **k))
    for i, (V, R, k) in enumerate(((51864, 1, 1), (51865, 3, 2), (51866, 8, 8), (51864, 5, 5), (3000, 2, 5), (2000, 4, 8),
                                   (64, 5, 8), (65, 6, 2), (70000, 7, 5), (256206, 2, 8), (256206, 4, 1))):
        add(f"random_v{V}_r{R}_k{k}", "random", 300 + i, R, V, k, None)
    for i, V in enumerate((51866, 256206, 65, 3000)):
        add(f"outlier_v{V}", "random", 320 + i, 2, V, 5, _outliers)
    add("all_equal_v51865", "tie", 330, 2, 51865, 8, _all_equal)
    add("all_equal_v256206", "tie", 331, 1, 256206, 5, _all_equal)
    for i, (V, k) in enumerate(((51864, 2), (51864, 5), (51866, 8), (256206, 8), (64, 8), (3000, 5))):
        add(f"few_finite_v{V}_k{k}", "tie", 340 + i, 3, V, k, _few_finite)
    for i, (V, k) in enumerate(((51866, 5), (51866, 8), (51864, 8), (70000, 5), (256206, 8), (3000, 8))):
        add(f"ties_across_v{V}_k{k}", "tie", 350 + i, 2, V, k, _ties_across(2))
        add(f"ties_thread_v{V}_k{k}", "tie", 360 + i, 2, V, k, _ties_same_thread)
        add(f"ties_edges_v{V}_k{k}", "tie", 370 + i, 2, V, k, _ties_slice_edges)
    for i, n in enumerate((1, 255, 256, 257, 1000)):
        add(f"adj_{n}", "random", 380 + i, 3, 51865, 5, None, _adj_unique(n))
    add("adj_1000_mixed_boundaries", "random", 390, 3, 51866, 5, None, _adj_unique(1000, True, True))
    add("adj_300_mixed_v256206", "random", 391, 2, 256206, 5, None, _adj_unique(300, True, True))
    add("adj_600_mixed_v3000", "random", 392, 4, 3000, 8, None, _adj_unique(600, True, True))
    add("adj_suppress_topk", "random", 393, 3, 51865, 5, None, _adj_suppress(False))
    add("adj_suppress_slice", "random", 394, 3, 51865, 8, None, _adj_suppress(True))
    add("adj_suppress_slice_v256206", "random", 395, 2, 256206, 5, None, _adj_suppress(True))
    add("nospeech_v51865_last_slice", "random", 400, 3, 51865, 2, None, None, ns=-2)
    add("nospeech_v51864", "random", 401, 1, 51864, 2, _outliers, None, ns=50362)
    add("nospeech_v70000", "random", 402, 2, 70000, 2, None, _adj_unique(40), ns=69999)
    return out


_ALIGN = dict(_align_cases())
_TOPK = dict(_topk_cases())
ALIGN_NAMES = list(_ALIGN)
TOPK_NAMES = list(_TOPK)


def build(name):
    return (_ALIGN.get(name) or _TOPK[name])()


def expected_routes(case):
    """the routes that must accept the case; every other one must answer WLK_ERR_ARG"""
    A, R, _, T = case["ring"].shape
    pre, ns, newest, _ = case["counters"]
    uniform = all(len(set(np.asarray(c).tolist())) == 1 for c in (pre, ns, newest, case["content_len"]))
    routes = [4]
    if uniform:
        routes += [0, 1]
        if A * T * 4 + 8192 + 1024 <= 150 * 1024:
            routes.append(2)
            if case["ns_token"] < 0:
                routes.append(3)
    return sorted(routes)
