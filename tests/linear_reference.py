"""Plain numpy reference of one linear layer as csrc/gemm_f32.hip computes it (GEMV and GEMM kernels, every epilogue
operand), for wlk_diag_linear_ex.

One function, `linear`, evaluates the whole operation in a given dtype, in a fixed order of steps:
  1 LayerNorm of the rows (eps 1e-5, biased variance)   2 A @ W.T   3 + bias
  4 scale: column c is multiplied by `scale` when c < scale_cols, or c % scale_period < scale_cols with a period
  5 exact-erf GELU   6 ReLU   7 x / (1 + exp(-x))   8 + R   9 the self-attention cache image after the append
float64 (`dt=np.float64`) is what the kernels are compared with; float32 (`dt=np.float32`, numpy float32 throughout) is
the restatement whose distance from the float64 form sizes the tolerance, nothing else.  `mutant` names a deliberate
mistake (tests/test_linear_reference_cpu.py shows that the cases tell each from the reference); the GPU tests never pass
one.  No torch in here.

Cache image (step 9): columns [kv_d, 2 kv_d) of an output row go to the K cache, [2 kv_d, 3 kv_d) to the V cache, at float
  shared caches, rows [beam][kv_ntok]:  ((row // kv_ntok) * kv_ctx + kv_pos + row % kv_ntok) * kv_d + col
  per-row caches (StepRow):             cache * cache_stride + kv_layer_off + offset * kv_d + col
  single row:                           kv_pos * kv_d + col     (the shared form with one beam and one token)

Tolerance (select_reference.value_tolerance, unchanged): a value may be off by KERNEL_FACTOR x the restatement's largest
error on the same case, floored at FLOOR * max(1, |reference|); OUTPUT_FACTOR below names the one family of outputs that
uses a measured factor instead."""
import math

import numpy as np

from select_reference import FLOOR, KERNEL_FACTOR, abs_err, value_tolerance  # noqa: F401  (the rule lives there)

GELU, RESIDUAL, SCALE, RELU, SWISH = 1, 2, 4, 8, 16          # GemmFlags (csrc/common.h)

MUTANTS = ("scale_boundary", "scale_no_period", "append_pos1", "append_ntok1", "steprow_row0", "ln_eps6", "ln_unbiased",
           "gelu_tanh", "residual_before_act", "bias_drop_last", "lda_is_k", "ldr_is_ldc", "k_tail_dropped",
           "tail_row_clamped")

# Factor that an output may use instead of KERNEL_FACTOR, keyed by kernel family (linear_cases.family): twice the largest
# kernel_err / restatement_err ratio measured on an MI355X over the whole table, rounded up to a power of two, for a kernel
# whose arithmetic was read and found right; profiles/linear_report_mi355x.json carries the ratio.  Never taken from the
# case it judges.
#   gemv_ln: the GEMV kernels' fused LayerNorm sums a row lane by lane (K / 64 terms in sequence, then a butterfly), the
#   order of layernorm_kernel.  On a row of mean 30 and spread 0.5 that mean lands a whole ulp of 30 (1.9e-6) from the
#   true one where numpy's pairwise float32 mean lands a tenth of that, and the offset goes through (x - mean) * rstd into
#   every feature: 3.3e-6 against the restatement's 5.3e-7 on row_k2048_n131_ln (ratio 6.13; the same order evaluated in
#   numpy float32 with the rest in double gives 2.7e-6).  2 x 6.13 -> 16.
OUTPUT_FACTOR = {"gemv_ln": 16.0}

_erf = np.frompyfunc(math.erf, 1, 1)


def _gelu(x, dt, tanh):
    x64 = x.astype(np.float64)
    if tanh:
        g = 0.5 * x64 * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x64 + 0.044715 * x64 ** 3)))
    else:
        g = 0.5 * x64 * (1.0 + _erf(x64 * 0.70710678118654752440).astype(np.float64))
    return g.astype(dt)       # (erf itself in double: the restatement rounds its result, as a correctly rounded erff would)


def scaled_columns(n, scale_cols, scale_period, mutant=None):
    """-> bool [n]: the columns step 4 multiplies"""
    col = np.arange(n)
    if scale_period and mutant != "scale_no_period":
        col = col % scale_period
    return col < (scale_cols + (1 if mutant == "scale_boundary" else 0))


def cache_indices(c, mutant=None):
    """-> int64 [m][kv_d] float index into kcache / vcache of column 0 .. kv_d - 1 of every row, or None without an append"""
    if not c["kv_mode"]:
        return None
    m, d = c["m"], c["kv_d"]
    row = np.arange(m)
    if c["kv_mode"] == 1:
        ntok = 1 if mutant == "append_ntok1" else c["kv_ntok"]
        pos = c["kv_pos"] + (1 if mutant == "append_pos1" else 0)
        base = ((row // ntok) * c["kv_ctx"] + pos + row % ntok) * d
    else:
        cache = np.array([r[0] for r in c["kv_rows"]])
        off = np.array([r[1] for r in c["kv_rows"]])
        if mutant == "steprow_row0":
            off = np.full_like(off, off[0])
        base = cache * c["cache_stride"] + c["kv_layer_off"] + off * d
    return base[:, None].astype(np.int64) + np.arange(d)[None, :]


def a_signal(c):
    """-> float32 [Z][(m - 1) lda + k]: the floats of every operand set of a as they lie in memory, rows lda apart -
    c["a_flat"] where the rows overlap (lda < k), else the rows of c["a"] with zeros between them"""
    if c.get("a_flat") is not None:
        return np.asarray(c["a_flat"], np.float32)
    z, m, k = c["a"].shape
    lda = c.get("lda") or k
    flat = np.zeros((z, (m - 1) * lda + k), np.float32)
    flat[:, np.arange(m)[:, None] * lda + np.arange(k)[None, :]] = c["a"]
    return flat


def _misread(flat, rows, cols, ld):
    """element (i, j) of every set taken from flat[i * ld + j] (wrapping at the end): rows read with the wrong stride"""
    return flat[:, (np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]) % flat.shape[1]]


def linear(c, dt=np.float64, mutant=None):
    """c: a case of tests/linear_cases.py or tests/gemm_tile_cases.py.  -> out [Z][m][n] in dt (Z = max(batch, 1)).
    c["a"] holds the rows whatever their distance in memory (with lda < k: a strided view of the flat signal)."""
    one = dt(1.0)
    a = np.asarray(c["a"], np.float32)                                    # [Z][m][k]
    if mutant == "lda_is_k":                                              # the rows read as if they lay k apart
        a = _misread(a_signal(c), c["m"], c["k"], c["k"])
    a = a.astype(dt)
    if mutant == "k_tail_dropped":                                        # the last k % 32 columns never reach the product
        a[..., c["k"] - c["k"] % 32:] = 0
    w = np.asarray(c["w"], np.float32).astype(dt)
    flags = c["flags"]
    with np.errstate(over="ignore", under="ignore"):
        if c["gamma"] is not None:
            k = a.shape[-1]
            mean = a.mean(axis=-1, keepdims=True, dtype=dt)
            dev = (a - mean).astype(dt)
            var = (dev * dev).sum(axis=-1, keepdims=True, dtype=dt) / dt(k - 1 if mutant == "ln_unbiased" else k)
            rstd = one / np.sqrt(var + dt(1e-6 if mutant == "ln_eps6" else 1e-5), dtype=dt)
            a = (dev * rstd * c["gamma"].astype(dt) + c["beta"].astype(dt)).astype(dt)
        y = np.matmul(a, w.T).astype(dt)
        if c["bias"] is not None:
            b = c["bias"].astype(dt)
            if mutant == "bias_drop_last":
                b = b.copy()
                b[-1] = 0
            y = (y + b).astype(dt)
        if flags & SCALE:
            cols = scaled_columns(c["n"], c["scale_cols"], c["scale_period"], mutant)
            y = np.where(cols, y * dt(np.float32(c["scale"])), y).astype(dt)
        res = c["r"].astype(dt) if flags & RESIDUAL else None
        if res is not None and mutant == "ldr_is_ldc":                    # r read with the rows of c's distance
            ldr, m, n = c["ldr"], c["m"], c["n"]
            flat = np.zeros((res.shape[0], m * ldr), dt)
            flat[:, np.arange(m)[:, None] * ldr + np.arange(n)[None, :]] = res
            res = _misread(flat, m, n, c["ldc"])
        if res is not None and mutant == "residual_before_act":
            y, res = (y + res).astype(dt), None
        if flags & GELU:
            y = _gelu(y, dt, mutant == "gelu_tanh")
        if flags & RELU:
            y = np.maximum(y, dt(0)).astype(dt)
        if flags & SWISH:
            y = (y / (one + np.exp(-y, dtype=dt))).astype(dt)
        if res is not None:
            y = (y + res).astype(dt)
        if mutant == "tail_row_clamped":                                  # the clamp of a tail row's loads leaking into its store
            y = y.copy()
            y[:, -1] = y[:, -2]
    return y


def cache_images(c, out, fill, mutant=None):
    """-> (kcache, vcache) [cache_floats] of out's dtype: `fill` everywhere but where step 9 writes row values of `out`
    (a mutant that writes behind the caches gets the longer image it needs)"""
    idx = cache_indices(c, mutant)
    if idx is None:
        return None, None
    d = c["kv_d"]
    size = max(c["cache_floats"], int(idx.max()) + 1)
    kc = np.full(size, fill, out.dtype)
    vc = np.full(size, fill, out.dtype)
    kc[idx.reshape(-1)] = out[0][:, d:2 * d].reshape(-1)
    vc[idx.reshape(-1)] = out[0][:, 2 * d:3 * d].reshape(-1)
    return kc, vc


def allowed_error(ref, f32, family=None):
    """-> (per-element allowed error, the restatement's own error): value_tolerance, with the family's factor if it has one"""
    allowed, e32 = value_tolerance(ref, f32)
    if family in OUTPUT_FACTOR:
        ref = np.asarray(ref, np.float64)
        mag = np.where(np.isfinite(ref), np.abs(ref), 0.0)
        allowed = np.maximum(OUTPUT_FACTOR[family] * e32, FLOOR * np.maximum(1.0, mag))
    return allowed, e32


def judge(name, got, ref, f32, family=None):
    """-> (report entry, failure text or None) for one output on one case"""
    allowed, e32 = allowed_error(ref, f32, family)
    err = abs_err(got, ref)
    worst = int(np.argmax(err - allowed))
    entry = dict(kernel_err=float(err.max()), restatement_err=e32, allowed=float(allowed.reshape(-1)[worst]),
                 of_allowed=float((err / allowed).max()))
    if family in OUTPUT_FACTOR:
        entry["output_factor"] = OUTPUT_FACTOR[family]
    fail = None
    if not np.all(np.isfinite(np.asarray(got, np.float64))):
        fail = f"{name}: not finite"
    elif (err > allowed).any():
        fail = (f"{name}: error {err.reshape(-1)[worst]:.3e} > allowed {allowed.reshape(-1)[worst]:.3e} "
                f"(restatement {e32:.3e}) at flat index {worst}")
    return entry, fail
