"""Plain numpy reference of the encoder operators wlk_diag_enc_op runs (csrc/gemm_x3.hip, layernorm.hip, attention.hip,
attention_x3.hip) and of the X3 format itself (csrc/x3.h).

The operators - `gemm`, `layernorm`, `attention` - evaluate the whole operation in a given dtype: float64 is what the
kernels are compared with; float32 (numpy float32 throughout) is the restatement whose distance from the float64 form
sizes the tolerance, nothing else.  `mutant` names a deliberate mistake (tests/test_enc_x3_reference_cpu.py shows that
the cases tell each from the reference); the GPU test never passes one.  No torch in here.

The X3 format: a float32 value as three bf16 planes hi, mid, lo, each the round-to-nearest-even bf16 of what the planes
before it left over (`split`).  A row image holds element (row, k), plane p at 16-bit word
    row * 3 * ld + (k // 8) * 24 + p * 8 + k % 8
and the attention operand image of T frames of a d-wide model is the row image [T][2 d] (q | k) followed, at word
T * 3 * 2 d, by V^T as a row image [d][vt_ld] (vt_ld = T rounded up to 32) whose stored position s of a row is key
32 (s // 32) + vt_key((s % 32) // 8, s % 8) - the order of ax_vt_key in csrc/attention_x3.hip.

Where the split is exact (x3.h; found by tests/test_enc_x3_reference_cpu.py): hi + mid + lo == x for every finite x with
|x| < SPLIT_OVERFLOW (from there on hi rounds to infinity) that is a multiple of 2^-133, the spacing of bf16's subnormals -
every float32 of magnitude 2^-110 or more is one; below that a value with bits under 2^-133 loses them (`split_exact`).

Tolerance (select_reference.value_tolerance, unchanged): a value may be off by KERNEL_FACTOR x the restatement's largest
error on the same case, floored at FLOOR * max(1, |reference|); OUTPUT_FACTOR below names the families of outputs that use
a measured factor instead."""
import math

import numpy as np

from select_reference import FLOOR, KERNEL_FACTOR, abs_err, value_tolerance  # noqa: F401  (the rule lives there)

GELU, RESIDUAL, SCALE = 1, 2, 4          # GemmFlags (csrc/common.h)
HEAD = 64

MUTANTS = ("residual_before_gelu", "scale_no_period", "scale_boundary4", "bias_next_quad", "ln_unbiased", "ln_eps_outside",
           "vt_plain_order", "drop_last_key", "pad_key_weight", "softmax_no_max", "session0_operand", "drop_lo")

# Factor that an output may use instead of KERNEL_FACTOR, keyed by kernel family (enc_x3_cases.family): twice the largest
# kernel_err / restatement_err ratio measured on an MI355X over the whole table, rounded up to a power of two, for a kernel
# whose arithmetic was read and found right; profiles/enc_x3_report_mi355x.json carries the ratios.  Never taken from the
# case it judges.
#   attention_pw: enc_attention_pw_kernel sums a score over its 64 features with 32 fp32 MFMAs in sequence, feature by
#   feature.  Where every score carries a common offset of 300 (one feature contributes 10 x 30) each of the 63 small terms
#   is rounded at the size of the running sum - ulp(300) = 3.1e-5 - where numpy's float32 matmul adds the small terms
#   among themselves first; exp() turns the score error into a relative error of the weights, and V reaches 60.  On
#   pw_t33_offset300 the kernel is 3.778e-3 off against the restatement's 5.287e-4 (ratio 7.15); the scores accumulated
#   feature by feature in numpy float32 with the rest in double give 3.781e-3 - the whole of it.  2 x 7.15 -> 16.
#   (enc_attention_x3_kernel keeps 4: its plane products are exact in the accumulator and the small ones come first - 1.0 x
#   the restatement on the same inputs.  The X3 GEMM, at most 2.12 x, and both LayerNorm kernels, at most 1.28 x, keep 4.)
OUTPUT_FACTOR = {"attention_pw": 16.0}

SPLIT_OVERFLOW = float(np.array([0x7F7F8000], np.uint32).view(np.float32)[0])      # 3.3961775e38: bf16(x) is infinite from here

_erf = np.frompyfunc(math.erf, 1, 1)


# ----------------------------------------------------------------------------------------------------------------------
# the format
# ----------------------------------------------------------------------------------------------------------------------
def bf16_bits(x):
    """float32 -> the bits of its round-to-nearest-even bf16 (on the bit pattern; finite inputs)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def bf16_value(bits):
    """bf16 bits -> float32"""
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def split(x):
    """float32 [...] -> uint16 [3][...]: the planes hi, mid, lo of x3_split (csrc/x3.h)"""
    x = np.ascontiguousarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        h = bf16_bits(x)
        r = x - bf16_value(h)
        m = bf16_bits(r)
        r2 = r - bf16_value(m)
        lo = bf16_bits(r2)
    return np.stack([h, m, lo])


def planes_value(planes):
    """uint16 [3][...] -> float64 hi + mid + lo (exact: three bf16 values span fewer than 53 bits wherever they are a split)"""
    p = bf16_value(planes).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (p[0] + p[1]) + p[2]


def split_exact(x):
    """-> bool [...]: x lies in the domain where hi + mid + lo == x (module docstring)"""
    x = np.ascontiguousarray(x, np.float32)
    x64 = np.abs(x.astype(np.float64))
    return np.isfinite(x) & (x64 < SPLIT_OVERFLOW) & (np.ldexp(x64, 133) == np.floor(np.ldexp(x64, 133)))


def drop_lo(x):
    """float32 -> float64 hi + mid: what a product sees when the lo plane is dropped"""
    p = bf16_value(split(x)).astype(np.float64)
    return p[0] + p[1]


def _row_words(rows, cols, ld):
    """-> int64 [rows][cols] word index of plane 0 of element (row, col) of a row image"""
    r = np.arange(rows, dtype=np.int64)[:, None]
    k = np.arange(cols, dtype=np.int64)[None, :]
    return r * 3 * ld + (k // 8) * 24 + k % 8


def pack_rows(x, ld, image=None, at=0):
    """float32 [rows][cols] -> the row image (rows 3 ld words apart) written into `image` at word `at` (a new one if None)"""
    x = np.ascontiguousarray(x, np.float32)
    rows, cols = x.shape
    if image is None:
        image = np.zeros(at + rows * 3 * ld, np.uint16)
    idx = at + _row_words(rows, cols, ld)
    planes = split(x)
    for p in range(3):
        image[idx + 8 * p] = planes[p]
    return image


def decode_rows(image, rows, cols, ld, at=0):
    """-> (value float64 [rows][cols], canonical bool [rows][cols]): hi + mid + lo of every element of a row image, and
    whether its three planes are the split of that value (a sum that is no float32, or planes split otherwise, are not)"""
    idx = at + _row_words(rows, cols, ld)
    planes = np.stack([np.asarray(image)[idx + 8 * p] for p in range(3)])
    value = planes_value(planes)
    with np.errstate(over="ignore", invalid="ignore"):
        as32 = value.astype(np.float32)
    as32 = np.where(value == 0, bf16_value(planes[0]), as32)          # (a sum of zeros has lost the sign that - 0 is split with)
    canonical = (as32.astype(np.float64) == value) & np.all(split(as32) == planes, axis=0)
    return value, canonical


def vt_key(u, e):
    """key (relative to its 32-key group) of element e of stored chunk u of V^T (ax_vt_key)"""
    return 4 * u + (e & 3) + 16 * (e >> 2)


def vt_ld(T):
    return (T + 31) // 32 * 32


def vt_off(T, d):
    return T * 3 * 2 * d


def attn_image_words(T, d):
    return vt_off(T, d) + d * 3 * vt_ld(T)


def vt_key_order(ld, plain=False):
    """-> int [ld]: the key that stored position s of a V^T row holds"""
    s = np.arange(ld)
    if plain:
        return s
    return 32 * (s // 32) + vt_key((s % 32) // 8, s % 8)


def pack_attn_image(qkv):
    """float32 qkv [T][3 d] -> the operand image of the X3 attention (pad keys are zeros)"""
    qkv = np.ascontiguousarray(qkv, np.float32)
    T, d = qkv.shape[0], qkv.shape[1] // 3
    ld = vt_ld(T)
    image = np.zeros(attn_image_words(T, d), np.uint16)
    pack_rows(qkv[:, :2 * d], 2 * d, image)
    v = np.zeros((ld, d), np.float32)
    v[:T] = qkv[:, 2 * d:]
    pack_rows(v[vt_key_order(ld)].T, ld, image, vt_off(T, d))
    return image


def decode_attn_image(image, T, d, plain_order=False):
    """-> (qk float64 [T][2 d], v float64 [vt_ld][d] in key order - the pad keys included -, canonical bool: every word)"""
    ld = vt_ld(T)
    qk, ok_qk = decode_rows(image, T, 2 * d, 2 * d)
    vt, ok_v = decode_rows(image, d, ld, ld, vt_off(T, d))
    v = np.empty((ld, d), np.float64)
    v[vt_key_order(ld, plain_order)] = vt.T
    return qk, v, bool(ok_qk.all() and ok_v.all())


def owned_words(kind, size, **kw):
    """-> bool [size]: the 16-bit words of an X3 result a launch must write; everything else keeps the guard.
    kind "rows": rows x cols at ld (the fc1 form, the LayerNorm image, the x3_out attention, the pack), at word `at`;
    kind "qkv": the attention operand image of T frames of a d-wide model, at word `at` - q | k rows AND all of V^T,
    the pad keys [T, vt_ld) included (the launch writes them as zeros)."""
    own = np.zeros(size, bool)
    at = kw.get("at", 0)
    if kind == "rows":
        idx = at + _row_words(kw["rows"], kw["cols"], kw["ld"])
        for p in range(3):
            own[idx + 8 * p] = True
    else:
        T, d = kw["T"], kw["d"]
        own |= owned_words("rows", size, rows=T, cols=2 * d, ld=2 * d, at=at)
        own |= owned_words("rows", size, rows=d, cols=vt_ld(T), ld=vt_ld(T), at=at + vt_off(T, d))
    return own


# ----------------------------------------------------------------------------------------------------------------------
# the operators
# ----------------------------------------------------------------------------------------------------------------------
def _gelu(x, dt):
    x64 = x.astype(np.float64)
    g = 0.5 * x64 * (1.0 + _erf(x64 * 0.70710678118654752440).astype(np.float64))
    return g.astype(dt)       # (erf itself in double: the restatement rounds its result, as a correctly rounded erff would)


def scaled_columns(n, scale_cols, scale_period, mutant=None):
    """-> bool [n]: the columns the scale multiplies: (col % period if period else col) < scale_cols"""
    col = np.arange(n)
    if scale_period and mutant != "scale_no_period":
        col = col % scale_period
    cols = col < scale_cols
    if mutant == "scale_boundary4":                 # a lane's four columns decided by the first of them
        q = 4 * (np.arange(n) // 4)
        cols = (q % scale_period if scale_period else q) < scale_cols
    return cols


def gemm(a, w, bias, flags=0, scale=1.0, scale_cols=0, scale_period=0, r=None, dt=np.float64, mutant=None):
    """a [..., m, k], w [n, k], bias [n] / None, r [..., m, n] / None -> epilogue(a w^T + bias) [..., m, n] in dt:
    + bias, x scale on the scaled columns, erf-GELU, + residual"""
    if mutant == "drop_lo":
        a, w = drop_lo(a), drop_lo(w)
    a = np.asarray(a).astype(dt)
    w = np.asarray(w).astype(dt)
    n = w.shape[0]
    with np.errstate(over="ignore", under="ignore"):
        y = np.matmul(a, w.T).astype(dt)
        if bias is not None:
            b = np.asarray(bias).astype(dt)
            if mutant == "bias_next_quad":
                b = np.roll(b, -4)
            y = (y + b).astype(dt)
        if flags & SCALE:
            y = np.where(scaled_columns(n, scale_cols, scale_period, mutant), y * dt(np.float32(scale)), y).astype(dt)
        res = np.asarray(r).astype(dt) if flags & RESIDUAL else None
        if res is not None and mutant == "residual_before_gelu":
            y, res = (y + res).astype(dt), None
        if flags & GELU:
            y = _gelu(y, dt)
        if res is not None:
            y = (y + res).astype(dt)
    return y


def layernorm(x, gamma, beta, dt=np.float64, mutant=None):
    """rows of x [..., d]: (x - mean) / sqrt(var + 1e-5) * gamma + beta, biased variance"""
    x = np.asarray(x).astype(dt)
    d = x.shape[-1]
    mean = x.mean(axis=-1, keepdims=True, dtype=dt)
    dev = (x - mean).astype(dt)
    var = (dev * dev).sum(axis=-1, keepdims=True, dtype=dt) / dt(d - 1 if mutant == "ln_unbiased" else d)
    if mutant == "ln_eps_outside":
        rstd = dt(1.0) / (np.sqrt(var, dtype=dt) + dt(1e-5))
    else:
        rstd = dt(1.0) / np.sqrt(var + dt(1e-5), dtype=dt)
    return (dev * rstd * np.asarray(gamma).astype(dt) + np.asarray(beta).astype(dt)).astype(dt)


def attention(qkv, n_head, dt=np.float64, mutant=None):
    """qkv [..., T, 3 d] (q and k already scaled) -> softmax(q k^T) v per 64-wide head, [..., T, d]"""
    qkv = np.asarray(qkv).astype(dt)
    T, d = qkv.shape[-2], qkv.shape[-1] // 3
    out = np.empty(qkv.shape[:-1] + (d,), dt)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for h in range(n_head):
            c = slice(HEAD * h, HEAD * (h + 1))
            q, k, v = qkv[..., c], qkv[..., d + HEAD * h:d + HEAD * (h + 1)], qkv[..., 2 * d + HEAD * h:2 * d + HEAD * (h + 1)]
            if mutant == "drop_last_key":
                k, v = k[..., :-1, :], v[..., :-1, :]
            if mutant == "pad_key_weight":          # one pad key (k = 0, v = 0) takes part: a score of 0
                zero = np.zeros(k.shape[:-2] + (1, HEAD), dt)
                k, v = np.concatenate([k, zero], -2), np.concatenate([v, zero], -2)
            s = np.matmul(q, np.swapaxes(k, -1, -2)).astype(dt)
            if mutant != "softmax_no_max":
                s = (s - s.max(axis=-1, keepdims=True)).astype(dt)
            p = np.exp(s, dtype=dt)
            out[..., c] = (np.matmul(p, v).astype(dt) / p.sum(axis=-1, keepdims=True, dtype=dt)).astype(dt)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# judging
# ----------------------------------------------------------------------------------------------------------------------
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
    kernel_err = float(err.max())
    entry = dict(kernel_err=kernel_err, restatement_err=e32, allowed=float(allowed.reshape(-1)[worst]),
                 of_allowed=float((err / allowed).max()), ratio=kernel_err / e32 if e32 > 0 else None,
                 factor=OUTPUT_FACTOR.get(family, KERNEL_FACTOR))
    fail = None
    if not np.all(np.isfinite(np.asarray(got, np.float64))):
        fail = f"{name}: not finite"
    elif (err > allowed).any():
        fail = (f"{name}: error {err.reshape(-1)[worst]:.3e} > allowed {allowed.reshape(-1)[worst]:.3e} "
                f"(restatement {e32:.3e}) at flat index {worst}")
    return entry, fail
