"""Named, seeded cases for wlk_diag_linear_ex (tests/test_gpu_linear.py) and their CPU checks
(tests/test_linear_reference_cpu.py).  SPECS holds the light description of every case; `case(name)` builds its arrays.

Single-row kernel (m = 1, route 1): every UB of gemv1_f32_kernel in its FULL and its predicated form (K = 256 UB and a K
below it), one and two features per wave (n = 131: the last workgroup has idle waves; n = 2049: the last pair has one live
feature), with and without the fused LayerNorm, and the plain UB 12 / 16 / 20 forms.  Staged kernel: every row bucket at
its limit, every RPW, the LayerNorm on both sides of the 512 features it keeps in registers, the grid-stride pass, both
cache forms.  GEMM kernels: scale_period, the prefill's cache append, operand tables.

Inputs are not one normal distribution: LayerNorm rows with mean 30 and spread 0.5, a constant row, a row of spread 0.01
(where eps matters), a zero weight row in every case, pre-activations spread over [-8, 8] where an activation follows (one
at -100 for swish), a residual a thousand times the product in one case."""
import zlib

import numpy as np

from linear_reference import GELU, RELU, RESIDUAL, SCALE, SWISH

SPECS = {}
REFUSED_SPECS = {}          # shapes no route takes: only tests/test_gpu_linear.py::test_refusals builds them
ROW_KINDS = ("normal", "mean30", "smallvar", "const")


def _add(name, m, n, k, routes=(1,), table=None, **kw):
    table = SPECS if table is None else table
    spec = dict(m=m, n=n, k=k, routes=tuple(routes), ln=False, bias=True, flags=0, scale=0.125, scale_cols=0,
                scale_period=0, r_is_c=False, kv_mode=0, kv_d=0, kv_pos=0, kv_ctx=0, kv_ntok=1, kv_rows=None, n_caches=0,
                kv_layer_off=0, batch=0, rows=("normal",), spread=False, res_scale=1.0, lda=0, ldr=0)
    assert name not in table and name not in SPECS and name not in REFUSED_SPECS and set(kw) <= set(spec), (name, kw)
    spec.update(kw)
    table[name] = spec


# ---- single-row kernel ------------------------------------------------------------------------------------------------
K_SMALL = (4, 132, 128, 384, 512, 640, 768, 896, 1024, 1152, 1280, 1408, 1536, 1792, 2048)      # UB 2 .. 8, FULL and not
K_WIDE = (2304, 3072, 3584, 4096, 4608, 5120)                                                   # UB 12 / 16 / 20
_EPILOGUES = (dict(), dict(flags=GELU, spread=True), dict(flags=RELU, spread=True), dict(flags=SWISH, spread=True),
              dict(flags=RESIDUAL), dict(flags=RESIDUAL, r_is_c=True), dict(flags=GELU | RESIDUAL, spread=True, r_is_c=True),
              dict(flags=SCALE, scale_cols=77))
_i = 0
for _k in K_SMALL:
    for _n in (131, 2049):
        for _ln in (False, True):
            _ep = _EPILOGUES[_i % len(_EPILOGUES)]
            _add(f"row_k{_k}_n{_n}_{'ln' if _ln else 'plain'}", 1, _n, _k, ln=_ln, bias=_i % 3 != 1 or "spread" in _ep,
                 rows=(ROW_KINDS[(_i // 2) % 3],), **_ep)
            _i += 1
for _k in K_WIDE:
    _ep = _EPILOGUES[_i % len(_EPILOGUES)]
    _add(f"row_k{_k}_n131_plain", 1, 131, _k, bias=_i % 3 != 1 or "spread" in _ep, **_ep)
    _i += 1
# q | k | v of a decode step: q and k scaled, k | v appended at a position that is neither 0 nor the last
_add("row_qkv_rpw1", 1, 3 * 384, 384, ln=True, flags=SCALE, scale_cols=2 * 384, kv_mode=1, kv_d=384, kv_ctx=7, kv_pos=3)
_add("row_qkv_rpw2", 1, 3 * 768, 768, ln=True, flags=SCALE, scale_cols=2 * 768, kv_mode=1, kv_d=768, kv_ctx=5, kv_pos=2)
# boundaries inside one wave's pair of features (RPW 2)
_add("row_odd_scale_cols", 1, 2049, 512, flags=SCALE, scale_cols=1001)
_add("row_odd_kv_d", 1, 3 * 683, 256, flags=SCALE, scale_cols=2 * 683, kv_mode=1, kv_d=683, kv_ctx=4, kv_pos=1, bias=False)
_add("row_swish_minus100", 1, 131, 512, flags=SWISH, spread=True)
_add("row_big_residual", 1, 131, 1280, flags=RESIDUAL, res_scale=1000.0, r_is_c=True)
_add("row_const_ln", 1, 131, 768, ln=True, rows=("const",))

# ---- staged kernel ----------------------------------------------------------------------------------------------------
_add("st_m2_n131_k5120", 2, 131, 5120, flags=RESIDUAL, r_is_c=True)                  # row-bucket limits: 64 KiB of LDS
_add("st_m4_n131_k4096", 4, 131, 4096, flags=GELU, spread=True)
_add("st_m8_n131_k2048", 8, 131, 2048, ln=True, rows=ROW_KINDS, flags=SWISH, spread=True)
_add("st_m3_n131_k132_ln", 3, 131, 132, ln=True, rows=ROW_KINDS)
_add("st_m5_n131_k512_ln", 5, 131, 512, ln=True, rows=ROW_KINDS, flags=RELU, spread=True)
_add("st_m2_n131_k576_ln", 2, 131, 576, ln=True, rows=("mean30", "smallvar"), bias=False)
_add("st_m1_n131_k2304_ln", 1, 131, 2304, ln=True, rows=("mean30",))                 # one row the single-row kernel cannot take
_add("st_m8_n32771_k128", 8, 32771, 128, flags=RESIDUAL)                             # RPW 4 and the grid-stride pass
_add("st_m1_n16385_k128", 1, 16385, 128, bias=False)
_add("st_m2_n16385_k128", 2, 16385, 128, flags=SCALE, scale_cols=16383)
_add("st_m4_n16385_k128", 4, 16385, 128, flags=RESIDUAL, r_is_c=True)
_add("st_m2_n2049_k512", 2, 2049, 512, flags=SCALE, scale_cols=1001)
_add("st_m3_n2049_k512", 3, 2049, 512, ln=True, rows=ROW_KINDS)
_add("st_m8_n2049_k132", 8, 2049, 132, flags=GELU, spread=True)
_add("st_qkv_3beams", 3, 3 * 384, 384, ln=True, rows=ROW_KINDS, flags=SCALE, scale_cols=2 * 384, kv_mode=1, kv_d=384, kv_ctx=6,
     kv_pos=2)
_add("st_qkv_odd_kv_d_2beams", 2, 3 * 683, 256, flags=SCALE, scale_cols=2 * 683 - 1, kv_mode=1, kv_d=683, kv_ctx=4, kv_pos=2)
_add("st_rows_m1", 1, 3 * 384, 384, ln=True, flags=SCALE, scale_cols=2 * 384, kv_mode=2, kv_d=384, kv_ctx=6, n_caches=2,
     kv_rows=((1, 4),), kv_layer_off=6 * 384)
_add("st_rows_m1_rpw2", 1, 3 * 768, 768, kv_mode=2, kv_d=768, kv_ctx=3, n_caches=1, kv_rows=((0, 1),), kv_layer_off=0)
_add("st_rows_m5_3caches", 5, 3 * 384, 384, ln=True, rows=ROW_KINDS, flags=SCALE, scale_cols=2 * 384, kv_mode=2, kv_d=384,
     kv_ctx=6, n_caches=3, kv_rows=((0, 1), (1, 4), (0, 3), (2, 0), (1, 2)), kv_layer_off=6 * 384)

# ---- GEMM kernels -----------------------------------------------------------------------------------------------------
# scale_period: n = 3 periods of 40 (171), 13 (37) scaled columns in each - no multiple of 16.  Smallest shapes each
# kernel takes: the k-wave kernels need K >= 256 (16 x 16 tiles up to 128 rows by shape), the k-pipe kernel K % 64 == 0,
# K >= 256 and 512 rows, the kp family K % 128 == 0
_P = dict(flags=SCALE, scale_cols=13, scale_period=40)
_add("gemm_period_32x64", 70, 120, 36, routes=(3,), **_P)
_add("gemm_period_64x64", 512, 513, 36, routes=(3,), flags=SCALE | RESIDUAL, scale_cols=37, scale_period=171)
_add("gemm_period_kwave", 40, 120, 256, routes=(2,), **_P)
_add("gemm_period_kwave16", 40, 120, 256, routes=(0,), **_P)
_add("gemm_period_kpipe", 512, 120, 256, routes=(4, 5), **_P)
_add("gemm_period_kp", 40, 120, 256, routes=(6, 7, 8), **_P)
# the decoder prefill's append: rows [beam][token]
_add("gemm_prefill_2x7", 14, 120, 256, routes=(0,), flags=SCALE, scale_cols=80, kv_mode=1, kv_d=40, kv_ctx=12, kv_pos=3, kv_ntok=7)
_add("gemm_prefill_2x70", 140, 120, 256, routes=(0,), flags=SCALE, scale_cols=80, kv_mode=1, kv_d=40, kv_ctx=75, kv_pos=3, kv_ntok=70)
# rows of a further apart than k and rows of r at another distance than the rows of c (lda, ldr: 0 = k, the distance of c's rows)
_add("gemm_strides_32x64", 37, 70, 36, routes=(3,), flags=RESIDUAL, lda=44, ldr=70 + 12)
# operand tables
_add("gemm_batch3_64x64", 512, 513, 36, routes=(3,), batch=3, flags=GELU | RESIDUAL, spread=True)
_add("gemm_batch3_kpipe", 512, 120, 256, routes=(4,), batch=3, flags=RESIDUAL, r_is_c=True)

# ---- refusals ---------------------------------------------------------------------------------------------------------
_add("x_period_row", 1, 131, 512, table=REFUSED_SPECS, **_P)
_add("x_batch_rows", 2, 131, 128, table=REFUSED_SPECS, batch=2)
_add("x_ln_gemm", 40, 120, 256, table=REFUSED_SPECS, ln=True)
_add("x_append_k36", 14, 120, 36, table=REFUSED_SPECS, kv_mode=1, kv_d=40, kv_ctx=12, kv_pos=3, kv_ntok=7)
_add("x_append_rows", 14, 120, 256, table=REFUSED_SPECS, kv_mode=1, kv_d=40, kv_ctx=12, kv_pos=3, kv_ntok=7)
_add("x_m9", 9, 131, 128, table=REFUSED_SPECS)
_add("x_k6", 1, 131, 6, table=REFUSED_SPECS)
# name -> (case the call is built from, call-level overrides, route, fragment of the message)
REFUSALS = {
    "scale_period on route 1": ("x_period_row", dict(), 1, "scale_period"),
    "batch on route 1": ("x_batch_rows", dict(), 1, "batched operand tables"),
    "LayerNorm on launch_gemm": ("x_ln_gemm", dict(), 3, "LayerNorm"),
    "LayerNorm on launch_gemm_kp": ("x_ln_gemm", dict(), 5, "LayerNorm"),
    "append on a GEMM shape that is not k-wave": ("x_append_k36", dict(), 0, "only available on the k-wave path"),
    "append on launch_gemm_kp": ("x_append_rows", dict(), 6, "plain projections only"),
    "m = 9 on route 1": ("x_m9", dict(), 1, "unsupported shape"),
    "k = 6 on route 1": ("x_k6", dict(), 1, "unsupported shape"),
    "k = 6 on launch_gemm": ("x_k6", dict(), 3, "multiples of 4"),
    "several tokens per row on route 1": ("x_append_rows", dict(), 1, "one token per row"),
    "per-row caches on a GEMM route": ("st_rows_m1", dict(), 0, "route 1"),
    "c too small": ("row_k128_n131_plain", dict(c_floats=130), 1, "rows of c lie past"),
    "caches too small": ("st_qkv_3beams", dict(kv_ctx=7), 1, "caches hold fewer"),
    "a row offset outside its cache": ("st_rows_m1", dict(kv_row_offset=[6]), 1, "kv_row_offset outside"),
    "an unknown route": ("row_k128_n131_plain", dict(route=9), 1, "route in [0, 8]"),
}

NAMES = tuple(SPECS)


def _rows(rng, kinds, z, m, k, ln):
    a = np.empty((z, m, k), np.float32)
    for i in range(z):
        for r in range(m):
            kind = kinds[(r + i) % len(kinds)] if ln else "normal"
            if kind == "normal":
                a[i, r] = rng.standard_normal(k)
            elif kind == "mean30":
                a[i, r] = 30.0 + 0.5 * rng.standard_normal(k)
            elif kind == "smallvar":
                a[i, r] = 0.01 * rng.standard_normal(k)
            else:
                a[i, r] = 2.5               # zero variance; K x 2.5 is exact in float32, so every summation order gives it
    return a


PAD = 4                                 # pad columns of the rows of c


def case(name):
    """-> the spec of `name` plus its arrays: a [Z][m][k], w [n][k], bias [n] / None, gamma, beta [k] / None, r [Z][m][n] /
    None (with r_is_c: what the output buffer holds on arrival), and the cache geometry"""
    return build(name, SPECS[name] if name in SPECS else REFUSED_SPECS[name])


def build(name, spec):
    """the arrays of spec `spec`, seeded by `name`.  lda = 0: the rows of a lie k (rounded up to 4) apart.  lda < k: the rows
    overlap - a_flat [Z][(m - 1) lda + k] is the signal and a its strided view.  ldr = 0: the rows of r lie as far apart as
    the rows of c (ldc = n + PAD)."""
    s = dict(spec)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    m, n, k = s["m"], s["n"], s["k"]
    z = max(s["batch"], 1)
    c = s
    c["name"] = name
    c["ldc"] = n + PAD
    c["ldr"] = c["ldc"] if s["r_is_c"] or not s["ldr"] else s["ldr"]
    if s["lda"] and s["lda"] < k:
        assert not s["ln"] and s["lda"] % 4 == 0, name
        c["a_flat"] = rng.standard_normal((z, (m - 1) * s["lda"] + k)).astype(np.float32)
        c["a"] = np.lib.stride_tricks.as_strided(c["a_flat"], (z, m, k), (c["a_flat"].strides[0], 4 * s["lda"], 4), writeable=False)
    else:
        c["a_flat"] = None
        c["a"] = _rows(rng, s["rows"], z, m, k, s["ln"])
    w = (rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32)
    if s["spread"]:
        w *= np.float32(0.25)
    w[n // 2] = 0.0                                             # a zero weight row: that output is its bias alone
    c["w"] = w
    bias = (0.5 * rng.standard_normal(n)).astype(np.float32)
    if s["spread"]:                                             # pre-activations over [-8, 8], whatever follows them
        bias = rng.permutation(np.linspace(-8.0, 8.0, n)).astype(np.float32)
        if s["flags"] & SWISH:
            bias[n // 2] = -100.0                               # (the zero weight row: the pre-activation is exactly -100)
        assert s["bias"], name
    c["bias"] = bias if s["bias"] else None
    if s["ln"]:
        c["gamma"] = (1.0 + 0.2 * rng.standard_normal(k)).astype(np.float32)
        c["beta"] = (0.1 * rng.standard_normal(k)).astype(np.float32)
    else:
        c["gamma"] = c["beta"] = None
    c["r"] = (s["res_scale"] * rng.standard_normal((z, m, n))).astype(np.float32) if s["flags"] & RESIDUAL else None
    if s["kv_mode"] == 1:
        c["cache_stride"] = 0
        c["cache_floats"] = (m // s["kv_ntok"]) * s["kv_ctx"] * s["kv_d"]
    elif s["kv_mode"] == 2:
        c["cache_stride"] = s["kv_layer_off"] + s["kv_ctx"] * s["kv_d"] + 4
        c["cache_floats"] = s["n_caches"] * c["cache_stride"]
    else:
        c["cache_stride"] = c["cache_floats"] = 0
    return c


def family(c, route):
    """the kernel family whose outputs route `route` of case c gives (linear_reference.OUTPUT_FACTOR is keyed by it)"""
    if route == 1 or (route == 0 and c["m"] <= 8):
        return "gemv_ln" if c["ln"] else "gemv"
    return "gemm"


def alone(c, z, row):
    """row `row` of operand set z of case c as a one-row case of its own, without the cache append"""
    s = dict(c)
    s.update(m=1, batch=0, kv_mode=0, kv_rows=None, cache_floats=0, cache_stride=0, name=f"{c['name']}[{z}][{row}]")
    s["a"] = c["a"][z:z + 1, row:row + 1]
    s["a_flat"], s["lda"] = None, 0
    s["r"] = c["r"][z:z + 1, row:row + 1] if c["r"] is not None else None
    return s


def mutants(c):
    """the deliberate mistakes of linear_reference.MUTANTS that change this case's result"""
    out = []
    f = c["flags"]
    if f & SCALE:
        out.append("scale_boundary")
        if c["scale_period"]:
            out.append("scale_no_period")
    if c["kv_mode"] == 1:
        out.append("append_pos1")
        if c["kv_ntok"] > 1:
            out.append("append_ntok1")
    if c["kv_mode"] == 2 and len({r[1] for r in c["kv_rows"]}) > 1:
        out.append("steprow_row0")
    if c["ln"]:
        out += ["ln_eps6", "ln_unbiased"]
    if f & GELU:
        out.append("gelu_tanh")
    if f & RESIDUAL and f & (GELU | RELU | SWISH):
        out.append("residual_before_act")
    if c["bias"] is not None:
        out.append("bias_drop_last")
    if c.get("lda") and c["lda"] != c["k"]:
        out.append("lda_is_k")
    if f & RESIDUAL and not c["r_is_c"] and c.get("ldr") and c["ldr"] != c["n"] + PAD:
        out.append("ldr_is_ldc")
    if c["k"] % 32:
        out.append("k_tail_dropped")
    if c["m"] >= 2:
        out.append("tail_row_clamped")
    return out
