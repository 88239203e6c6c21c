"""Inputs of the csrc/sortformer.hip kernel tests: one generator module for test_sf_kernel_reference_cpu.py (which checks the
references and the cases' power to tell mistakes apart) and test_gpu_sf_kernels.py (which runs them through
wlk_diag_sf_kernel).  Everything is seeded by the case's name; nothing is read from a file.

Attention inputs are sharp on purpose: content scores of standard deviation ~3, a relative-position term of comparable
size from random (non-sinusoidal) rows, one loud value channel - a softmax over nearly flat scores would average an
indexing mistake away."""
import zlib

import numpy as np

MAX_FRAMES = 512
ATTN_T = (1, 2, 15, 16, 17, 33, 49, 64, 65, 113, 193, 291, 401, 512)
EIGHT = (512, 1, 16, 17, 33, 64, 113, 2)
GAP = 2                     # NaN rows in front of every segment


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ----------------------------------------------------------------------------------------------------------------------
# attention
# ----------------------------------------------------------------------------------------------------------------------
ATTENTION = {}


def _attn(name, T, dh, pos_row0=None, H=2, bias="", scale="rsqrt", segs=None, planted=False):
    assert name not in ATTENTION
    ATTENTION[name] = dict(name=name, T=T, dh=dh, pos_row0=pos_row0, H=H, bias=bias, scale=scale, segs=segs, planted=planted)


for _T in ATTN_T:
    _attn(f"t{_T}_dh64_nopos", _T, 64)                                           # the NLLB encoder
    _attn(f"t{_T}_dh24_nopos", _T, 24, scale="one")                              # the Transformer blocks
    _attn(f"t{_T}_dh64_pos_edge", _T, 64, pos_row0=_T - 1, bias="uv")            # rbase < 0 on the last tile, clamps at both ends
    _attn(f"t{_T}_dh64_pos_511", _T, 64, pos_row0=511, bias="uv")                # the Conformer blocks
for _dh in (24, 40, 4, 60):                                                      # dead chunks of both templates
    _attn(f"dead_t113_dh{_dh}_nopos", 113, _dh, scale="one" if _dh == 24 else "rsqrt")
    _attn(f"dead_t113_dh{_dh}_pos_edge", 113, _dh, pos_row0=112, bias="uv")
_attn("t291_dh40_pos_511", 291, 40, pos_row0=511, bias="uv")
for _b in ("", "u", "v"):
    _attn(f"t49_dh64_pos_edge_bias_{_b or 'none'}", 49, 64, pos_row0=48, bias=_b)
_attn("t49_dh64_nopos_bias_u", 49, 64, bias="u")
_attn("t65_dh64_pos_edge_scale_one", 65, 64, pos_row0=64, bias="uv", scale="one")
_attn("t33_dh24_pos_511_h8", 33, 24, pos_row0=511, H=8, bias="uv")
_attn("planted_t49_dh64_edge", 49, 64, pos_row0=48, bias="v", scale="one", planted=True)
_attn("planted_t291_dh24_511", 291, 24, pos_row0=511, bias="v", scale="one", planted=True)
for _n, _lens in (("seg1", (65,)), ("seg3", (291, 17, 1)), ("seg8", EIGHT)):
    _attn(f"{_n}_dh64_pos_511", max(_lens), 64, pos_row0=511, bias="uv", segs=_lens)
    _attn(f"{_n}_dh64_nopos", max(_lens), 64, segs=_lens)
    _attn(f"{_n}_dh24_nopos", max(_lens), 24, scale="one", segs=_lens)
_attn("seg3_dh40_pos_edge", 291, 40, pos_row0=290, bias="uv", segs=(291, 17, 1))
ATTENTION_NAMES = list(ATTENTION)
PLANT_OFFSET = 3


def attention_case(name):
    """-> dict: q / k / v [rows][H][dh] float32 (NaN in the gap rows of a segmented case), pos [2 pos_row0 + 1][H][dh] (NaN
    outside the rows T can reach) or None, bias_u / bias_v [H][dh] or None, scale, segs [(start, T)] or None"""
    c = dict(ATTENTION[name])
    rng = _rng(name)
    T, dh, H = c["T"], c["dh"], c["H"]
    scale = np.float32(1.0 / np.sqrt(np.float32(dh))) if c["scale"] == "rsqrt" else np.float32(1.0)
    amp = np.sqrt(3.0 / (float(scale) * np.sqrt(dh)))           # q, k ~ amp N(0, 1): content scores of std ~3
    if c["segs"] is None:
        rows, spans = T, None
    else:
        spans, at = [], 0
        for n in c["segs"]:
            spans.append((at + GAP, n))
            at += GAP + n
        rows = at
    q, k, v = (rng.standard_normal((rows, H, dh)) for _ in range(3))
    q *= amp
    k *= amp
    v[:, 0, dh - 1] *= 30.0                                      # the loud channel: the last live column of head 0
    pos = bias_u = bias_v = None
    if "u" in c["bias"]:
        bias_u = (0.7 * amp * rng.standard_normal((H, dh))).astype(np.float32)
    if "v" in c["bias"]:
        bias_v = (0.7 * amp * rng.standard_normal((H, dh))).astype(np.float32)
    if c["pos_row0"] is not None:
        r0 = c["pos_row0"]
        pos = 0.7 * amp * rng.standard_normal((2 * r0 + 1, H, dh))
    plant = None
    if c["planted"]:
        # q = 0, no u, k small: score[i][j] = bias_v . pos[pos_row0 - i + j]; the rows at offsets 0 .. 3 are aligned with
        # bias_v, 30 apart, so row i peaks at the largest offset it can reach: j = min(i + 3, T - 1)
        q[:] = 0.0
        k *= 0.01 / amp
        pos *= 0.1 / (0.7 * amp)
        bias_v = rng.standard_normal((H, dh)).astype(np.float32)
        for o in range(PLANT_OFFSET + 1):
            for h in range(H):
                pos[c["pos_row0"] + o, h] = 30.0 * (o + 1) * bias_v[h] / float(np.dot(bias_v[h].astype(np.float64), bias_v[h]))
        plant = np.minimum(np.arange(T) + PLANT_OFFSET, T - 1)
    q, k, v = (a.astype(np.float32) for a in (q, k, v))
    if spans is not None:
        owned = np.zeros(rows, bool)
        for a, n in spans:
            owned[a:a + n] = True
        for a in (q, k, v):
            a[~owned] = np.nan
    if pos is not None:
        pos = pos.astype(np.float32)
        r0 = c["pos_row0"]
        pos[:r0 - (T - 1)] = np.nan
        pos[r0 + T:] = np.nan
    c.update(q=q, k=k, v=v, pos=pos, bias_u=bias_u, bias_v=bias_v, scale=scale, segs=spans, rows=rows, plant=plant)
    return c


def attention_mutants(case):
    """the mistakes of sf_kernel_reference.ATTENTION_MUTANTS this case can tell from the reference"""
    c = case
    longest = max(n for _, n in c["segs"]) if c["segs"] else c["T"]
    out = []
    if longest >= 2:
        out.append("drop_last_key")
        if c["pos"] is not None:
            out.append("rel_off_by_one")
            if float(c["scale"]) != 1.0:
                out.append("scale_content_only")
        if c["bias_u"] is not None or c["bias_v"] is not None:
            out.append("swap_uv")
    if c["segs"] and len(c["segs"]) >= 2:
        out.append("seg_neighbour")
    return out


def attention_alone(case, s):
    """segment s of a segmented case as a case of its own (n_seg = 0, the same table and pos_row0)"""
    a, n = case["segs"][s]
    c = dict(case, name=f"{case['name']}[{s}]", T=n, rows=n, segs=None, q=np.ascontiguousarray(case["q"][a:a + n]),
             k=np.ascontiguousarray(case["k"][a:a + n]), v=np.ascontiguousarray(case["v"][a:a + n]))
    return c


# ----------------------------------------------------------------------------------------------------------------------
# the stem's convolutions: (session input lengths, F, C)
# ----------------------------------------------------------------------------------------------------------------------
CONV = {
    "one_1_f128_c256": ((1,), 128, 256),
    "one_2_f9_c96": ((2,), 9, 96),
    "one_8_f8_c320": ((8,), 8, 320),
    "one_9_f1_c96": ((9,), 1, 96),
    "one_101_f128_c256": ((101,), 128, 256),
    "one_101_f9_c320": ((101,), 9, 320),
    "three_f128_c96": ((101, 1, 9), 128, 96),
    "three_f1_c320": ((8, 1, 2), 1, 320),
    "eight_f9_c256": ((8, 1, 101, 2, 9, 1, 101, 2), 9, 256),
    "eight_f8_c320": ((101, 1, 101, 9, 8, 2, 1, 1), 8, 320),
}
CONV_NAMES = list(CONV)


def conv_case(kind, name):
    """kind 'conv0': x [sum lens][F], w [C][9]; 'dwconv2d': x [sum lens][F][C], w [9][C]"""
    lens, F, C = CONV[name]
    rng = _rng(kind + name)
    n = sum(lens)
    x = rng.standard_normal((n, F) if kind == "conv0" else (n, F, C)).astype(np.float32)
    w = (rng.standard_normal((C, 9) if kind == "conv0" else (9, C)) / 3.0).astype(np.float32)
    b = (0.3 * rng.standard_normal(C)).astype(np.float32)
    return dict(name=name, kind=kind, lens=lens, F=F, C=C, x=x, w=w, b=b)


# ----------------------------------------------------------------------------------------------------------------------
# the Conformer convolution core: (session lengths, d, taps)
# ----------------------------------------------------------------------------------------------------------------------
GLU = {
    "one_1_d512_k9": ((1,), 512, 9),
    "one_3_d130_k9": ((3,), 130, 9),
    "one_3_d512_k31": ((3,), 512, 31),
    "one_37_d130_k31": ((37,), 130, 31),
    "one_291_d512_k9": ((291,), 512, 9),
    "one_291_d130_k31": ((291,), 130, 31),
    "three_d512_k31": ((37, 1, 291), 512, 31),
    "eight_d130_k9": ((3, 37, 1, 291, 3, 1, 37, 3), 130, 9),
    "eight_d512_k31": ((37, 3, 1, 37, 3, 291, 1, 3), 512, 31),
}
GLU_NAMES = list(GLU)


def glu_case(name):
    lens, d, taps = GLU[name]
    rng = _rng("glu" + name)
    n = sum(lens)
    x = rng.standard_normal((n, 2 * d)).astype(np.float32)
    w = (rng.standard_normal((taps, d)) / np.sqrt(taps / 4.0)).astype(np.float32)
    b, bn_b = ((0.3 * rng.standard_normal(d)).astype(np.float32) for _ in range(2))
    # a running mean well away from 0, so that its sign matters on every channel
    bn_mean = (rng.choice([-1.0, 1.0], d) * (0.5 + rng.random(d))).astype(np.float32)
    bn_invstd = (0.5 + rng.random(d)).astype(np.float32)
    bn_w = (rng.choice([-1.0, 1.0], d) * (0.5 + rng.random(d))).astype(np.float32)
    return dict(name=name, lens=lens, d=d, taps=taps, x=x, w=w, b=b, bn_mean=bn_mean, bn_invstd=bn_invstd, bn_w=bn_w, bn_b=bn_b)


# ----------------------------------------------------------------------------------------------------------------------
# the head: (T, d, n_spk); the assembly: [(context rows, chunk rows)] per session
# ----------------------------------------------------------------------------------------------------------------------
HEAD = {f"t{T}_d{d}_s{s}": (T, d, s) for T, d, s in ((1, 192, 4), (5, 200, 5), (293, 192, 4), (293, 200, 5), (5, 192, 5))}
HEAD_NAMES = list(HEAD)


def head_case(name):
    T, d, n_spk = HEAD[name]
    rng = _rng("head" + name)
    return dict(name=name, T=T, d=d, n_spk=n_spk, x=rng.standard_normal((T, d)).astype(np.float32),
                w1t=(rng.standard_normal((d, d)) / np.sqrt(d / 2.0)).astype(np.float32), b1=(0.3 * rng.standard_normal(d)).astype(np.float32),
                w2=(rng.standard_normal((n_spk, d)) * (1.5 / np.sqrt(d))).astype(np.float32), b2=(0.5 * rng.standard_normal(n_spk)).astype(np.float32))


ASSEMBLE = {
    "one_300_25": [(300, 25)],
    "one_0_25": [(0, 25)],
    "one_1_0": [(1, 0)],
    "three": [(300, 25), (0, 25), (1, 0)],
    "eight": [(1, 25), (0, 0), (300, 0), (0, 25), (1, 0), (300, 25), (1, 25), (0, 25)],
}
ASSEMBLE_NAMES = list(ASSEMBLE)
ASSEMBLE_D = 512


def assemble_case(name):
    sess = ASSEMBLE[name]
    rng = _rng("assemble" + name)
    lens, chunk_lens = [a + b for a, b in sess], [b for _, b in sess]
    ctx_rows = rng.standard_normal((sum(lens), ASSEMBLE_D)).astype(np.float32)
    at = 0
    for n, nc in zip(lens, chunk_lens):        # the chunk positions of the context buffer hold nothing a session may read
        ctx_rows[at + n - nc:at + n] = np.nan
        at += n
    chunk_rows = rng.standard_normal((sum(chunk_lens), ASSEMBLE_D)).astype(np.float32)
    return dict(name=name, lens=lens, chunk_lens=chunk_lens, d=ASSEMBLE_D, ctx_rows=ctx_rows, chunk_rows=chunk_rows,
                scale=np.float32(np.sqrt(np.float32(ASSEMBLE_D))))
