"""Named, seeded cases for wlk_diag_enc_op (tests/test_gpu_enc_x3.py) and their CPU checks
(tests/test_enc_x3_reference_cpu.py).  SPECS holds the light description of every case; `case(name)` builds its arrays and
`reference(case, dt, mutant)` evaluates it with tests/enc_x3_reference.py.

Shapes are the smallest that reach an edge of the kernels, not the workload's: the X3 GEMM (csrc/gemm_x3.hip) one row off
either tile height, N off the 128-column tile and off the 32-row weight block, K = 2, 4, 6 and 10 slabs against the five
ring slots, the banded walk with empty slots, persistent workgroups that skip a slot between two tiles, every epilogue
operand run_encode_group (csrc/api.hip) passes, operand tables of 1, 2, 3, 5 and 8 sessions at unequal offsets, both X3
result forms; the LayerNorm kernels in every NPL instantiation; both encoder attention kernels around their tile sizes.

Inputs are not one normal distribution: LayerNorm rows with mean 30 and spread 0.5, a constant row, a row of spread 0.01, a
zero weight row in every GEMM, pre-activations spread over [-8, 8] where GELU follows, a residual a thousand times the
product, attention scores with one key 60 above the rest, a common offset of 300, or all equal."""
import zlib

import numpy as np

import enc_x3_reference as ER
from enc_x3_reference import GELU, RESIDUAL, SCALE

SPECS = {}
REFUSED_SPECS = {}          # shapes no launcher takes: only tests/test_gpu_enc_x3.py::test_refusals builds them
ROW_KINDS = ("normal", "mean30", "smallvar", "const")
ATT_KINDS = ("model", "qrow6", "offset300", "equal", "dominant_first", "dominant_last", "dominant_other")
ENV_KEYS = ("WLK_X3_BM", "WLK_X3_PERSIST", "WLK_X3_COLMAJOR")
ALL_WALKS = tuple((bm, p, c) for bm in (96, 64) for p in (1, 0) for c in (1, 0))        # the first one is judged
BOTH_HEIGHTS = ((96, 1, 1), (64, 1, 0))
CUS = 256                   # compute units of the target: what wlk_diag_x3_plan is asked about

# tile sizes of enc_attention_pw_kernel (csrc/attention.hip: QT, KT, NWAVE) and enc_attention_x3_kernel (AX_QT, AX_KT)
PW_QT, PW_KT, PW_NWAVE = 32, 32, 4
AX_QT, AX_KT = 64, 32
LN_MAX_D = 64 * 24          # kLnMaxPerLane (csrc/layernorm.hip)


def _add(name, kind, table=None, **kw):
    table = SPECS if table is None else table
    base = dict(kind=kind, batch=0, form=0)
    if kind == "gemm":
        base.update(m=0, n=0, k=0, flags=0, bias=True, scale=0.125, scale_cols=0, scale_period=0, r_is_c=False, spread=False,
                    res_scale=1.0, walks=ALL_WALKS, d=0)
    elif kind == "ln":
        base.update(rows=0, d=0, kinds=ROW_KINDS)
    elif kind == "attention":
        base.update(T=0, H=1, inputs="model")
    else:
        base.update(rows=0, cols=0)
    assert name not in SPECS and name not in REFUSED_SPECS and set(kw) <= set(base), (name, kw)
    base.update(kw)
    table[name] = base


# ---- X3 GEMM, fp32 result: every M, N, K of the edge sets, the epilogues dealt round ------------------------------------
GEMM_M = (1, 63, 64, 65, 95, 96, 97)
GEMM_N = (4, 124, 128, 132, 1028)
GEMM_K = (64, 128, 192, 320)
EPILOGUES = {
    "bias": dict(),
    "nobias": dict(bias=False),
    "gelu": dict(flags=GELU, spread=True),
    "res": dict(flags=RESIDUAL),
    "resc": dict(flags=RESIDUAL, r_is_c=True),
    "geluresc": dict(flags=GELU | RESIDUAL, r_is_c=True, spread=True),
    "scale6": dict(flags=SCALE, scale_cols=6),
    "scale6p10": dict(flags=SCALE, scale_cols=6, scale_period=10),
    "bigres": dict(flags=RESIDUAL, r_is_c=True, res_scale=1000.0),
}
_i = 0
for _a, _m in enumerate(GEMM_M):
    for _b, _n in enumerate(GEMM_N):
        _k = GEMM_K[(_a + _b) % len(GEMM_K)]
        _e = list(EPILOGUES)[_i % len(EPILOGUES)]
        _add(f"g_m{_m}_n{_n}_k{_k}_{_e}", "gemm", m=_m, n=_n, k=_k, **EPILOGUES[_e])
        _i += 1
# the production pair of dec_cross_kv_x3: scale_cols = d, scale_period = 2 d (two decoder layers of a d = 64 model), with a table
_add("g_crosskv_d64", "gemm", m=97, n=256, k=64, batch=3, flags=SCALE, scale=0.3535533905932738, scale_cols=64, scale_period=128)
# banded walk (eight or more tile rows): 769 rows are nine 96-row tiles - the fourth row band is empty - and thirteen 64-row
# tiles - the fourth row band holds one; N = 1152 is nine tile columns, the second column band one short
_add("g_banded", "gemm", m=769, n=1152, k=64, flags=RESIDUAL, r_is_c=True)
_add("g_banded_b2", "gemm", m=769, n=1152, k=64, batch=2, flags=GELU, spread=True)
# a persistent workgroup that walks three tiles and more and skips an empty slot between two of them (wlk_diag_x3_plan at
# 256 CUs says so: tests/test_enc_x3_reference_cpu.py); the output is the residual of every session
_add("g_banded_b5_skip", "gemm", m=769, n=1152, k=64, batch=5, flags=RESIDUAL, r_is_c=True,
     walks=((96, 1, 0), (64, 1, 0), (96, 0, 0), (64, 0, 1), (96, 1, 1)))
# plain walk, more tiles than workgroups: 2 x 18 x 8 = 288 on 256
_add("g_plain_b8_two_tiles", "gemm", m=97, n=2304, k=64, batch=8)
# operand tables at unequal offsets
_add("g_table_b1", "gemm", m=97, n=132, k=128, batch=1, flags=RESIDUAL)
_add("g_table_b2", "gemm", m=65, n=1028, k=64, batch=2, flags=SCALE, scale_cols=6, scale_period=10)
_add("g_table_b3_alias", "gemm", m=97, n=132, k=192, batch=3, flags=RESIDUAL, r_is_c=True)
_add("g_table_b8", "gemm", m=63, n=124, k=128, batch=8, flags=GELU | RESIDUAL, r_is_c=True, spread=True)
# a production width: enc_out_x3 of a d = 1024 model on 97 frames
_add("g_out_d1024", "gemm", m=97, n=1024, k=1024, batch=1, flags=RESIDUAL, r_is_c=True, walks=BOTH_HEIGHTS)
# ---- the fc1 form: GELU, every column to the row image fc2 reads ----------------------------------------------------------
_add("fc1_m33_n128", "gemm", form=1, m=33, n=128, k=64, flags=GELU, spread=True, walks=BOTH_HEIGHTS)
_add("fc1_m96_n256_b3", "gemm", form=1, m=96, n=256, k=128, batch=3, flags=GELU, spread=True, walks=BOTH_HEIGHTS)
_add("fc1_m97_n1152", "gemm", form=1, m=97, n=1152, k=64, flags=GELU, spread=True, walks=BOTH_HEIGHTS)
_add("fc1_m97_n128_b3", "gemm", form=1, m=97, n=128, k=192, batch=3, flags=GELU, spread=True, walks=BOTH_HEIGHTS)
# ---- the qkv form: q | k rows and V^T, the operand image of the X3 attention (n = 3 d, k = d, q | k scaled) ----------------
for _d, _t, _bz in ((64, 33, 0), (64, 64, 3), (128, 70, 0), (128, 97, 3), (384, 97, 0), (384, 64, 0), (64, 97, 0), (128, 33, 3)):
    _add(f"qkv_d{_d}_t{_t}_b{_bz}", "gemm", form=2, d=_d, m=_t, n=3 * _d, k=_d, batch=_bz, flags=SCALE, scale=0.3535533905932738,
         scale_cols=2 * _d, walks=BOTH_HEIGHTS)

# ---- LayerNorm: every NPL instantiation (8, 12, 16, 20 and kLnMaxPerLane = 24: d up to 1536), four rows per workgroup --------
LN_D = (8, 64, 384, 520, 776, 1032, 1280, 1288, LN_MAX_D)
for _i, _d in enumerate(LN_D):
    _add(f"ln_d{_d}", "ln", d=_d, rows=(1, 3, 4, 5)[_i % 4], batch=(0, 1, 3, 8)[(_i + 1) % 4])
_add("ln_d384_r5_b8", "ln", d=384, rows=5, batch=8)
_add("ln_d1288_r4", "ln", d=1288, rows=4, batch=0)
_add("ln_d520_r1_b3", "ln", d=520, rows=1, batch=3, kinds=("mean30",))

# ---- attention ---------------------------------------------------------------------------------------------------------
PW_T = (1, PW_QT - 1, PW_QT, PW_QT + 1, PW_NWAVE * PW_KT - 1, PW_NWAVE * PW_KT, PW_NWAVE * PW_KT + 1)
for _i, _t in enumerate(PW_T):
    _add(f"pw_t{_t}", "attention", form=0, T=_t, H=1 + _i % 3, batch=(0, 1, 3, 8)[_i % 4], inputs=ATT_KINDS[_i % len(ATT_KINDS)])
_add("pw_t129_dominant_last", "attention", form=0, T=129, H=1, inputs="dominant_last")
_add("pw_t33_offset300", "attention", form=0, T=33, H=2, batch=3, inputs="offset300")
AX_T = (64, 65, 95, 96, 97, 127, 128, 129, 193)
for _i, _t in enumerate(AX_T):
    _add(f"ax_t{_t}", "attention", form=1, T=_t, H=1 + _i % 3, batch=(0, 1, 3, 8)[(_i + 2) % 4], inputs=ATT_KINDS[_i % len(ATT_KINDS)])
# the dominant key in turn at key 0, at key T - 1 (inside the partial last tile) and in the other stream's tile: three key
# tiles (the partial one in stream 0) and four (in stream 1)
for _t in (65, 97):
    for _w in ("dominant_first", "dominant_last", "dominant_other"):
        if f"ax_t{_t}" in SPECS and SPECS[f"ax_t{_t}"]["inputs"] == _w:
            continue
        _add(f"ax_t{_t}_{_w}", "attention", form=1, T=_t, H=2, inputs=_w)
_add("ax_t129_equal_b3", "attention", form=1, T=129, H=1, batch=3, inputs="equal")
_add("ax_t97_offset300", "attention", form=1, T=97, H=3, inputs="offset300")

# ---- pack --------------------------------------------------------------------------------------------------------------
_add("pack_1x8", "pack", rows=1, cols=8)
_add("pack_5x72", "pack", rows=5, cols=72)
_add("pack_random_bits", "pack", rows=64, cols=64)

# ---- refusals: name -> (case the call is built from, call-level overrides, fragment of the message) --------------------------
_add("x_k32", "gemm", table=REFUSED_SPECS, m=8, n=128, k=32)
_add("x_k96", "gemm", table=REFUSED_SPECS, m=8, n=128, k=96)
_add("x_n6", "gemm", table=REFUSED_SPECS, m=8, n=6, k=64)
_add("x_n132_fc1", "gemm", table=REFUSED_SPECS, form=1, m=33, n=132, k=64, flags=GELU, spread=True)
_add("x_res_fc1", "gemm", table=REFUSED_SPECS, form=1, m=33, n=128, k=64, flags=RESIDUAL)
_add("x_ax_t63", "attention", table=REFUSED_SPECS, form=1, T=63, H=1)
# the fragments are the LAUNCHERS' texts (x3_gemm_check, enc_attention_x3_check: the functions the launchers themselves call)
# except for the last entry, which is the diagnostic's own buffer check; every call fails exactly one predicate
REFUSALS = {
    "K = 32": ("x_k32", dict(), "x3 gemm: K must be a multiple of 64, lda of 8"),
    "K = 96": ("x_k96", dict(), "x3 gemm: K must be a multiple of 64, lda of 8"),
    "lda % 8 != 0": ("g_m63_n124_k192_scale6", dict(ld_in=196), "x3 gemm: K must be a multiple of 64, lda of 8"),
    "N = 6": ("x_n6", dict(), "x3 gemm: N, ldc and ldr must be multiples of 4"),
    "ldc % 4 != 0": ("g_m63_n124_k192_scale6", dict(ld_out=126), "x3 gemm: N, ldc and ldr must be multiples of 4"),
    "misaligned bias": ("g_m63_n124_k192_scale6", dict(bias_off=2), "x3 gemm: bias, C and R must be 16-byte aligned"),
    "misaligned bias with a table": ("g_table_b8", dict(bias_off=2), "x3 gemm: bias must be 16-byte aligned"),
    "residual with an X3 result": ("x_res_fc1", dict(), "x3 gemm: unsupported X3 result layout"),
    "vt_col0 % 128 != 0": ("qkv_d64_t33_b0", dict(vt_col0=64), "x3 gemm: unsupported X3 result layout"),
    "vt_ld < M": ("qkv_d64_t97_b0", dict(vt_ld=96), "x3 gemm: unsupported X3 result layout"),
    "batch = 9": ("g_table_b8", dict(batch=9), "batch in [0, 8]"),
    # the contract settled for an X3 result with N % 8 != 0: the row image is stored in whole 8-column
    # chunks, so launch_gemm_x3 refuses the shape instead of writing four values that belong to no column (ldc3 = 144,
    # vt_col0 = 256: nothing else about the call is refused)
    "X3 result with N = 132": ("x_n132_fc1", dict(), "x3 gemm: an X3 result needs N % 8 == 0"),
    "X3 attention at T = 63": ("x_ax_t63", dict(), "x3 attention: unsupported shape"),
    "result too small": ("g_m63_n124_k192_scale6", dict(out_floats=100), "rows of c lie past"),
}

NAMES = tuple(SPECS)
GEMM_NAMES = tuple(n for n in NAMES if SPECS[n]["kind"] == "gemm")
LN_NAMES = tuple(n for n in NAMES if SPECS[n]["kind"] == "ln")
ATT_NAMES = tuple(n for n in NAMES if SPECS[n]["kind"] == "attention")
PACK_NAMES = tuple(n for n in NAMES if SPECS[n]["kind"] == "pack")


def _ln_rows(rng, kinds, z, rows, d):
    x = np.empty((z, rows, d), np.float32)
    for i in range(z):
        for r in range(rows):
            kind = kinds[(r + i) % len(kinds)]
            if kind == "normal":
                x[i, r] = rng.standard_normal(d)
            elif kind == "mean30":
                x[i, r] = 30.0 + 0.5 * rng.standard_normal(d)
            elif kind == "smallvar":
                x[i, r] = 0.01 * rng.standard_normal(d)
            else:
                x[i, r] = 2.5               # zero variance; d x 2.5 is exact in float32, so every summation order gives it
    return x


def dominant_key(T, where):
    """the key that is 60 above the rest: 0, T - 1 (inside the partial last tile) or inside the tile before the last one
    (the other key stream of the X3 kernel, another wave of the fp32 one)"""
    if where == "dominant_first":
        return 0
    if where == "dominant_last":
        return T - 1
    n_tiles = (T + AX_KT - 1) // AX_KT
    return max(0, AX_KT * (n_tiles - 2) + 5)


def _qkv(rng, inputs, z, T, H):
    d = ER.HEAD * H
    q = (0.6 * rng.standard_normal((z, T, d))).astype(np.float32)
    k = (0.6 * rng.standard_normal((z, T, d))).astype(np.float32)
    v = rng.standard_normal((z, T, d)).astype(np.float32)
    v[..., 5] *= 20.0                                    # a loud V channel
    first = np.arange(H) * ER.HEAD                       # feature 0 of every head carries what a case adds to the scores
    if inputs == "qrow6":
        q[:, T // 2] *= 6.0
    elif inputs.startswith("dominant"):
        q *= 0.5
        k *= 0.5
        q[..., first] = 6.0
        k[..., first] = 0.0
        k[:, dominant_key(T, inputs), first] = 10.0      # that key's score is 60 above the others'
    elif inputs == "offset300":
        q[..., first] = 10.0
        k[..., first] = 30.0                             # + 300 on every score of every row
    elif inputs == "equal":
        k[:] = 0.0                                       # every score is 0: the output is the mean of V
    return np.concatenate([q, k, v], axis=-1)


PACK_EDGE = np.array([0x00000000, 0x80000000, 0x3F800000, 0x3F800001, 0x00800000, 0x00000001, 0x00400000, 0x007FFFFF,
                      0x00800001, 0x08800001, 0x7F7E0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0xFF7FFFFF, 0x04010203],
                     np.uint32)
# (+-0, 1, 1 + 2^-23, 2^-126, three subnormals, 2^-126 (1 + 2^-23) and 2^-110 (1 + 2^-23) - their remainder planes are
# subnormal, the first one's is lost -, 3.38e38, the last value below the overflow of hi, the first one in it, +-FLT_MAX, one
# more that loses its lo plane)


def case(name):
    """-> the spec of `name` plus its arrays (Z = max(batch, 1) operand sets):
    gemm: a [Z][m][k], w [n][k], bias [n] / None, r [Z][m][n] / None;  ln: x [Z][rows][d], gamma, beta [d];
    attention: qkv [Z][T][3 d];  pack: x [rows][cols]"""
    s = dict(SPECS[name] if name in SPECS else REFUSED_SPECS[name])
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    z = max(s["batch"], 1)
    s["name"] = name
    if s["kind"] == "gemm":
        m, n, k = s["m"], s["n"], s["k"]
        s["a"] = rng.standard_normal((z, m, k)).astype(np.float32)
        w = (rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32)
        if s["spread"]:
            w *= np.float32(0.25)
        w[n // 2] = 0.0                                             # a zero weight row: that output is its bias alone
        s["w"] = w
        bias = (0.5 * rng.standard_normal(n)).astype(np.float32)
        if s["spread"]:                                             # pre-activations over [-8, 8] in front of GELU
            bias = rng.permutation(np.linspace(-8.0, 8.0, n)).astype(np.float32)
            assert s["bias"], name
        s["bias"] = bias if s["bias"] else None
        s["r"] = (s["res_scale"] * rng.standard_normal((z, m, n))).astype(np.float32) if s["flags"] & RESIDUAL else None
    elif s["kind"] == "ln":
        d = s["d"]
        s["x"] = _ln_rows(rng, s["kinds"], z, s["rows"], d)
        s["gamma"] = (1.0 + 0.2 * rng.standard_normal(d)).astype(np.float32)
        s["beta"] = (0.1 * rng.standard_normal(d)).astype(np.float32)
    elif s["kind"] == "attention":
        s["d"] = ER.HEAD * s["H"]
        s["qkv"] = _qkv(rng, s["inputs"], z, s["T"], s["H"])
    else:
        rows, cols = s["rows"], s["cols"]
        if name == "pack_random_bits":                              # a few thousand bit patterns of finite floats
            bits = rng.integers(0, 1 << 32, rows * cols, dtype=np.uint64).astype(np.uint32)
            bits[(bits & 0x7F800000) == 0x7F800000] &= np.uint32(0xBFFFFFFF)
            x = bits.view(np.float32)
        else:
            x = rng.standard_normal(rows * cols).astype(np.float32)
            x[:min(PACK_EDGE.size, x.size)] = PACK_EDGE.view(np.float32)[:x.size]
            if x.size > PACK_EDGE.size:
                x[-PACK_EDGE.size:] = PACK_EDGE.view(np.float32)
        s["x"] = x.reshape(rows, cols).copy()
    return s


def reference(c, dt=np.float64, mutant=None):
    """-> the output [Z][...] of case c in dt (tests/enc_x3_reference.py), under a deliberate mistake if `mutant` names one"""
    def operand(x):         # "session z reads session 0's operand"
        return np.broadcast_to(x[:1], x.shape) if mutant == "session0_operand" else x
    if c["kind"] == "gemm":
        return ER.gemm(operand(c["a"]), c["w"], c["bias"], c["flags"], c["scale"], c["scale_cols"], c["scale_period"], c["r"], dt, mutant)
    if c["kind"] == "ln":
        return ER.layernorm(operand(c["x"]), c["gamma"], c["beta"], dt, mutant)
    if c["kind"] == "attention":
        if mutant == "vt_plain_order":          # the image's V^T rows read back with the keys in plain order
            out = []
            for qkv in c["qkv"]:
                qk, v, _ = ER.decode_attn_image(ER.pack_attn_image(qkv), c["T"], c["d"], plain_order=True)
                out.append(ER.attention(np.concatenate([qk, v[:c["T"]]], axis=-1), c["H"], dt))
            return np.stack(out)
        return ER.attention(operand(c["qkv"]), c["H"], dt, mutant)
    raise ValueError(c["kind"])


def family(c):
    """the kernel family of a case's outputs (enc_x3_reference.OUTPUT_FACTOR is keyed by it)"""
    if c["kind"] == "attention":
        return "attention_x3" if c["form"] == 1 else "attention_pw"
    return c["kind"]


def mutants(c):
    """the deliberate mistakes of enc_x3_reference.MUTANTS that bear on this case"""
    out = []
    if c["kind"] == "gemm":
        out.append("drop_lo")
        f = c["flags"]
        if f & GELU and f & RESIDUAL:
            out.append("residual_before_gelu")
        if f & SCALE:
            out.append("scale_boundary4")
            if c["scale_period"]:
                out.append("scale_no_period")
        if c["bias"] is not None:
            out.append("bias_next_quad")
    elif c["kind"] == "ln":
        out += ["ln_unbiased", "ln_eps_outside"]
    elif c["kind"] == "attention":
        out += ["pad_key_weight", "softmax_no_max"] + (["drop_last_key"] if c["T"] > 1 else [])
        if c["form"] == 1:
            out.append("vt_plain_order")
    if c["batch"] > 1:
        out.append("session0_operand")
    return out


def plan(lib, c, walk, cus=CUS):
    """wlk_diag_x3_plan's text for GEMM case c under walk = (WLK_X3_BM, _PERSIST, _COLMAJOR), or with none of the switches
    set (walk = None: the default geometry); restores the environment"""
    import ctypes
    import os
    old = {key: os.environ.get(key) for key in ENV_KEYS}
    try:
        for key, val in zip(ENV_KEYS, walk or (None, None, None)):
            if val is None:
                os.environ.pop(key, None)
            else:
                os.environ[key] = str(val)
        lib.wlk_diag_env_refresh()
        buf = ctypes.create_string_buffer(320)
        rc = lib.wlk_diag_x3_plan(c["m"], c["n"], c["k"], c["batch"], cus, buf, 320)
        assert rc == 0, buf.value
        return dict(kv.split("=") if "=" in kv else (kv, "1") for kv in buf.value.decode().split())
    finally:
        for key, val in old.items():
            if val is None:
                os.environ.pop(key, None)
            else:
                os.environ[key] = val
        lib.wlk_diag_env_refresh()
