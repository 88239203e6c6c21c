"""Inputs of the decoder-attention tests: one generator module for test_dec_attention_reference_cpu.py (which checks the
references on these very cases) and test_gpu_dec_attention.py (which runs them through wlk_diag_dec_attention).

A self-attention case (kind "self"): n_rows, n_tok, d, H, ctx_len, offsets [1] or [n_rows], qkv [n_rows n_tok][3 d],
kc / vc [cache rows][ctx_len][d] (zeros at and behind every row's key count), form:
  "plain"  one offset; S0 takes it, and - one token per row - S1 (identity rows) and S2 (identity table, <= 8 rows) too
  "rows"   per-row offsets and cache rows, a non-zero layer_off: S1
  "anc"    an ancestry table: S2;  anc_alt = a table that differs only where it must not matter
A cross-attention case (kind "cross"): R, d, H, T, q, k / v [n_kv][T][d], row_kv, head_rank (or None), n_align, n_beam,
ring_rows, ring_row, beam_of_row, routes (the routes that take it), and the operands of C2 (x, wq, bq, gamma, beta, scale)
and C3 (wo, bo, resid) where those routes are listed.
`refused` maps a route to a fragment of the message it must refuse the case with."""
import numpy as np

HEAD = 64
SPLIT = 8                   # kCrossSplit of decoder.hip
QK_SCALE = 64 ** -0.25


def _rng(name):
    return np.random.default_rng(abs(hash_name(name)))


def hash_name(name):
    h = 2166136261
    for ch in name.encode():
        h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
    return h


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


# ----------------------------------------------------------------------------------------------------------------------
# self-attention
# ----------------------------------------------------------------------------------------------------------------------
def _self_case(name, n_rows, n_tok, offsets, d=128, H=2, ctx_len=448, form="plain", cache_rows=None, row_cache=None,
               anc=None, anc_alt=None, targets=None, refused=None):
    rng = _rng(name)
    offsets = np.atleast_1d(np.asarray(offsets, np.int32))
    cache_rows = cache_rows or n_rows
    qkv = _f32(rng.standard_normal((n_rows * n_tok, 3 * d)) * QK_SCALE)
    kc = _f32(rng.standard_normal((cache_rows, ctx_len, d)) * QK_SCALE)
    vc = _f32(rng.standard_normal((cache_rows, ctx_len, d)))
    if targets is not None:             # one query row: key j of head h scores targets[j] (up to rounding)
        assert n_rows == 1 and n_tok == 1
        for h in range(H):
            qh = qkv[0, h * HEAD:(h + 1) * HEAD].astype(np.float64)
            kc[0, :len(targets), h * HEAD:(h + 1) * HEAD] = _f32(np.asarray(targets)[:, None] * qh[None, :] / (qh @ qh))
    c = dict(name=name, kind="self", n_rows=n_rows, n_tok=n_tok, d=d, H=H, ctx_len=ctx_len, offsets=offsets, qkv=qkv, form=form,
             row_cache=None if row_cache is None else np.asarray(row_cache, np.int32), anc=anc, anc_alt=anc_alt,
             layer_off=1028 if form == "rows" else 0, refused=refused or {})
    # nothing at or behind a row's key count is part of the operation: zeros there (the stale runs replace them)
    c["key_count"] = np.zeros(cache_rows, np.int64)
    for b in range(n_rows):
        row = b if row_cache is None else int(row_cache[b])
        c["key_count"][row] = int(offsets[b] if len(offsets) > 1 else offsets[0]) + n_tok
    if form == "anc":
        c["key_count"][:] = int(offsets[0]) + 1           # every physical row may be read up to the key count
    for row in range(cache_rows):
        kc[row, c["key_count"][row]:] = 0
        vc[row, c["key_count"][row]:] = 0
    c["kc"], c["vc"] = kc, vc
    return c


def stale(case, fill):
    """the case with `fill` in every cache position at or behind its row's key count"""
    c = dict(case)
    c["kc"], c["vc"] = case["kc"].copy(), case["vc"].copy()
    for row, n in enumerate(case["key_count"]):
        c["kc"][row, n:] = fill
        c["vc"][row, n:] = fill
    return c


KEY_COUNTS = (1, 2, 4, 5, 32, 33, 127, 128, 129, 255, 256, 257, 447, 448)
PREFILLS = tuple((t, r) for t in (2, 3, 37, 129) for r in (1, 3))
ANC_KINDS = (("random", 2, 200), ("random", 5, 60), ("random", 7, 300), ("random", 8, 129), ("identity", 5, 200),
             ("shared", 7, 140), ("tail255", 5, 200), ("clamp", 5, 200), ("clamp", 8, 447))


def _anc_table(kind, n_rows, offset, ctx_len, rng):
    count = offset + 1
    own = np.tile(np.arange(n_rows, dtype=np.uint8)[:, None], (1, ctx_len))
    if kind == "identity":
        return own, None
    anc = own.copy()
    if kind == "shared":
        anc[:, :count] = n_rows - 2
    else:
        anc[:, :count] = rng.integers(0, n_rows, (n_rows, count))
    alt = None
    if kind == "tail255":
        alt = anc.copy()
        anc[:, count:] = 255
    if kind == "clamp":                 # entries at or above n_rows in front of the key count read the last row
        alt = anc.copy()
        hit = rng.random((n_rows, count)) < 0.2
        hit[:, [0, count - 1, min(128, count - 1)]] = True
        big = rng.integers(n_rows, 256, (n_rows, count)).astype(np.uint8)
        big[:, 0] = 255
        anc[:, :count] = np.where(hit, big, anc[:, :count])
        alt[:, :count] = np.where(hit, n_rows - 1, alt[:, :count])
    return anc, alt


def _self_builders():
    b = {}
    for n in KEY_COUNTS:
        b[f"keys_{n}"] = lambda name, n=n: _self_case(name, 2, 1, n - 1)
    for t, r in PREFILLS:
        b[f"prefill_t{t}_r{r}"] = lambda name, t=t, r=r: _self_case(name, r, t, 5)
    b["ctx24_keys11"] = lambda name: _self_case(name, 2, 1, 10, ctx_len=24)
    b["ctx24_keys24"] = lambda name: _self_case(name, 2, 1, 23, ctx_len=24)
    b["ctx512_keys512"] = lambda name: _self_case(name, 2, 1, 511, ctx_len=512)
    b["ctx513_refused"] = lambda name: _self_case(name, 2, 1, 100, ctx_len=513,
                                                  refused={r: "context too long" for r in ("S0", "S1", "S2")})
    b["d384_h6"] = lambda name: _self_case(name, 2, 1, 40, d=384, H=6)
    b["d1024_h16_nllb"] = lambda name: _self_case(name, 2, 1, 130, d=1024, H=16, ctx_len=256)
    b["rows8"] = lambda name: _self_case(name, 8, 1, [0, 447, 1, 127, 128, 129, 300, 33], form="rows", cache_rows=8,
                                         row_cache=[3, 0, 7, 1, 6, 2, 5, 4])
    for kind, n_rows, off in ANC_KINDS:
        def make(name, kind=kind, n_rows=n_rows, off=off):
            anc, alt = _anc_table(kind, n_rows, off, 448, _rng(name + "/table"))
            return _self_case(name, n_rows, 1, off, form="anc", anc=anc, anc_alt=alt)
        b[f"anc_{kind}_{n_rows}_o{off}"] = make
    n = 300
    peak = np.random.default_rng(5).standard_normal(n)
    peak[171] += 80.0
    b["val_dominant80"] = lambda name: _self_case(name, 1, 1, n - 1, targets=peak)
    b["val_all_equal"] = lambda name: _self_case(name, 1, 1, n - 1, targets=np.full(n, 0.5))
    pm = np.where(np.arange(n) % 3 == 0, 60.0, -60.0) + np.random.default_rng(6).standard_normal(n)
    b["val_pm60"] = lambda name: _self_case(name, 1, 1, n - 1, targets=pm)
    return b


# ----------------------------------------------------------------------------------------------------------------------
# cross-attention
# ----------------------------------------------------------------------------------------------------------------------
def _cross_case(name, R, T, routes, d=128, heads="one", n_beam=1, n_kv=1, fold=None, proj=False, targets=None, refused=None):
    """heads: "none" | "one" | "all" alignment heads.  fold = (bias?, scale) adds the operands of C2, proj those of C3."""
    rng = _rng(name)
    H = d // HEAD
    q = _f32(rng.standard_normal((R, d)) * QK_SCALE)
    k = _f32(rng.standard_normal((n_kv, T, d)) * QK_SCALE)
    v = _f32(rng.standard_normal((n_kv, T, d)))
    if targets is not None:
        assert R == 1 and n_kv == 1
        for h in range(H):
            qh = q[0, h * HEAD:(h + 1) * HEAD].astype(np.float64)
            k[0, :, h * HEAD:(h + 1) * HEAD] = _f32(np.asarray(targets)[:, None] * qh[None, :] / (qh @ qh))
    c = dict(name=name, kind="cross", R=R, d=d, H=H, T=T, q=q, k=k, v=v, n_kv=n_kv, routes=list(routes), refused=refused or {},
             row_kv=rng.integers(0, n_kv, R).astype(np.int32), head_rank=None, n_align=0, n_beam=n_beam, ring_rows=R + 3,
             ring_row=None, beam_of_row=None, bq=None)
    if n_kv > 1:
        c["row_kv"][:min(R, n_kv)] = np.arange(min(R, n_kv))[::-1]
    if heads != "none":
        ranks = np.full(H, -1, np.int32)
        if heads == "one":
            c["n_align"] = 3
            ranks[H - 1] = 1
        else:
            c["n_align"] = H + 1
            ranks[:] = rng.permutation(H + 1)[:H]
        c["head_rank"] = ranks
        # rows of one beam land in distinct ring rows; beams are dealt round robin through a permutation
        c["beam_of_row"] = (rng.permutation(n_beam)[np.arange(R) % n_beam]).astype(np.int32)
        c["ring_row"] = rng.permutation(c["ring_rows"])[:R].astype(np.int32)
    if fold is not None:
        bias, scale = fold
        c["x"] = _f32(rng.standard_normal((R, d)) * 2 + 0.3)
        c["wq"] = _f32(rng.standard_normal((d, d)) / np.sqrt(d))
        c["bq"] = _f32(rng.standard_normal(d) * 0.5) if bias else None
        c["gamma"] = _f32(1 + 0.2 * rng.standard_normal(d))
        c["beta"] = _f32(0.2 * rng.standard_normal(d))
        c["scale"] = float(np.float32(scale))
    if proj:
        c["wo"] = _f32(rng.standard_normal((d, d)) / np.sqrt(d))
        c["bo"] = _f32(rng.standard_normal(d) * 0.5)
        c["resid"] = _f32(rng.standard_normal(d) * 2)
    return c


STEP = ("C0", "C1", "C4")
STEP1 = ("C0", "C1", "C3", "C4")        # one row: the merged out projection too


def _value_targets(kind):
    T = 1500
    chunk = (T + SPLIT - 1) // SPLIT    # 188
    t = np.random.default_rng(11).standard_normal(T)
    if kind.startswith("dom"):
        t[int(kind[3:])] += 80.0
    elif kind == "equal":
        t[:] = 0.25
    elif kind.startswith("slice_low"):  # 60 below: the slice's rescale factor is ~1e-26; 120 below: it underflows to 0
        t[3 * chunk:4 * chunk] -= float(kind[9:])
    return t


def _cross_builders():
    b = {}
    # T and rows of the step forms
    b["step_T1500_r1_one"] = lambda n: _cross_case(n, 1, 1500, STEP1, heads="one", proj=True)
    b["step_T1500_r8_all_b3"] = lambda n: _cross_case(n, 8, 1500, STEP, heads="all", n_beam=3)
    b["step_T1536_r2_none"] = lambda n: _cross_case(n, 2, 1536, STEP, heads="none")
    b["step_T1497_r7_all"] = lambda n: _cross_case(n, 7, 1497, STEP, heads="all")
    b["step_T64_r2_one_b3"] = lambda n: _cross_case(n, 2, 64, STEP, heads="one", n_beam=3)
    b["step_T57_r1_all"] = lambda n: _cross_case(n, 1, 57, STEP1, heads="all", proj=True)
    b["step_T1500_r7_kv3"] = lambda n: _cross_case(n, 7, 1500, ("C4",), heads="one", n_beam=3, n_kv=3)
    # one-pass kernel beyond the step forms
    b["onepass_T1500_r9_all_b3"] = lambda n: _cross_case(n, 9, 1500, ("C0",), heads="all", n_beam=3)
    b["onepass_T64_r16_one"] = lambda n: _cross_case(n, 16, 64, ("C0",), heads="one")
    # prefill (flash) form: k_splits 1 and the default on every case
    b["prefill_T1500_r9_all_b3"] = lambda n: _cross_case(n, 9, 1500, ("C5",), heads="all", n_beam=3)
    b["prefill_T64_r32_one"] = lambda n: _cross_case(n, 32, 64, ("C5",), heads="one")
    b["prefill_T1500_r33_none"] = lambda n: _cross_case(n, 33, 1500, ("C5",), heads="none")
    b["prefill_T1536_r65_one"] = lambda n: _cross_case(n, 65, 1536, ("C5",), heads="one")
    # folded query projection
    b["fold_d256_r1_bias_s"] = lambda n: _cross_case(n, 1, 1500, ("C2",), d=256, heads="one", fold=(True, QK_SCALE))
    b["fold_d256_r8_nobias_1"] = lambda n: _cross_case(n, 8, 64, ("C2",), d=256, heads="all", fold=(False, 1.0))
    b["fold_d512_r2_bias_1"] = lambda n: _cross_case(n, 2, 64, ("C2",), d=512, heads="one", fold=(True, 1.0))
    b["fold_d768_r7_nobias_s"] = lambda n: _cross_case(n, 7, 64, ("C2",), d=768, heads="none", fold=(False, QK_SCALE))
    b["fold_d1280_r2_bias_s"] = lambda n: _cross_case(n, 2, 57, ("C2",), d=1280, heads="one", fold=(True, QK_SCALE))
    b["fold_d384_refused"] = lambda n: _cross_case(n, 1, 64, (), d=384, heads="none", fold=(True, 1.0),
                                                   refused={"C2": "cannot fold"})
    # merged out projection: wave form (d <= 512), LDS form (768, 1280); zero, one and H alignment heads
    b["merge_d128_none"] = lambda n: _cross_case(n, 1, 1500, ("C1", "C3"), d=128, heads="none", proj=True)
    b["merge_d384_all"] = lambda n: _cross_case(n, 1, 1500, ("C1", "C3"), d=384, heads="all", proj=True)
    b["merge_d512_one"] = lambda n: _cross_case(n, 1, 64, ("C1", "C3"), d=512, heads="one", proj=True)
    b["merge_d768_all"] = lambda n: _cross_case(n, 1, 1500, ("C1", "C3"), d=768, heads="all", proj=True)
    b["merge_d1280_one"] = lambda n: _cross_case(n, 1, 64, ("C1", "C3"), d=1280, heads="one", proj=True)
    b["merge_d1280_none"] = lambda n: _cross_case(n, 1, 57, ("C1", "C3"), d=1280, heads="none", proj=True)
    b["merge_rows2_refused"] = lambda n: _cross_case(n, 2, 64, ("C1",), heads="one", proj=True, refused={"C3": "single-row"})
    # values
    for kind in ("dom100", "dom1400", "dom187", "dom188", "equal", "slice_low60", "slice_low120"):
        b[f"val_{kind}"] = lambda n, kind=kind: _cross_case(n, 1, 1500, STEP1, heads="all", proj=True, targets=_value_targets(kind))
    # shapes a route must refuse
    b["T1537_refused"] = lambda n: _cross_case(n, 1, 1537, (), heads="none",
                                               refused={"C0": "T too large", "C1": "T too large", "C4": "T too large"})
    b["T1540_refused"] = lambda n: _cross_case(n, 1, 1540, (), heads="none", refused={"C0": "T too large", "C1": "T too large"})
    b["T9_refused"] = lambda n: _cross_case(n, 1, 9, ("C0",), heads="none", refused={"C1": "T too small", "C4": "T too small"})
    b["T1497_dump_refused"] = lambda n: _cross_case(n, 9, 1497, (), heads="one", refused={"C5": "Tk % 4"})
    return b


SELF_BUILDERS = _self_builders()
CROSS_BUILDERS = _cross_builders()
SELF_NAMES = sorted(SELF_BUILDERS)
CROSS_NAMES = sorted(CROSS_BUILDERS)


def build(name):
    return (SELF_BUILDERS.get(name) or CROSS_BUILDERS[name])(name)


def expected_routes(case):
    """the routes that must take the case (every route in case["refused"] must refuse it)"""
    if case["kind"] == "cross":
        return list(case["routes"])
    if case["refused"]:
        return []
    if case["form"] == "rows":
        return ["S1"]
    if case["form"] == "anc":
        return ["S2"]
    return ["S0"] + (["S1", "S2"] if case["n_tok"] == 1 and case["n_rows"] <= 8 else [])


# ----------------------------------------------------------------------------------------------------------------------
# ancestry sequences (A0) and what the beam routes do with them
# ----------------------------------------------------------------------------------------------------------------------
def anc_sequence(name, n_rows, ctx_len, first_offset, n_steps, rewind_at=None):
    """-> list of (ctl [8], offset): the first step is fresh, every later one continues random survivors; offsets grow by
    one per step, except at step `rewind_at`, which falls back by three positions"""
    rng = _rng(name)
    seq, off = [], first_offset
    for u in range(n_steps):
        ctl = np.zeros(8, np.int32)
        ctl[:n_rows] = np.arange(n_rows) if u == 0 else rng.integers(0, n_rows, n_rows)
        ctl[7] = 1 if u == 0 else 0
        if rewind_at is not None and u == rewind_at:
            off -= 3
        seq.append((ctl, off))
        off += 1
    return seq


ANC_SEQUENCES = {
    "seq_r2": dict(n_rows=2, ctx_len=448, first_offset=4, n_steps=9),
    "seq_r5": dict(n_rows=5, ctx_len=448, first_offset=126, n_steps=8),
    "seq_r7": dict(n_rows=7, ctx_len=448, first_offset=250, n_steps=10, rewind_at=6),
    "seq_r7_ctx24": dict(n_rows=7, ctx_len=24, first_offset=3, n_steps=12),
    "seq_r3_ctx512": dict(n_rows=3, ctx_len=512, first_offset=505, n_steps=7),
    "seq_r1": dict(n_rows=1, ctx_len=448, first_offset=0, n_steps=3),
}
