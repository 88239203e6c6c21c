"""CPU checks of the encoder-operator reference (tests/enc_x3_reference.py) and its case table (tests/enc_x3_cases.py):
the reference equals torch double, the float32 restatement stays inside its own tolerance, the X3 split is exact on the
domain x3.h states and not outside it, the table reaches every route it claims (asserted through wlk_diag_x3_plan at 256
compute units), and every deliberate mistake pushes at least one named case out of tolerance.  No GPU."""
import numpy as np
import pytest
import torch

import enc_x3_cases as EC
import enc_x3_reference as ER
from whisperlivekit_amd import _lib

_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = EC.case(name)
    return _CASES[name]


_REFS = {}


def refs(name):
    if name not in _REFS:
        c = case(name)
        _REFS[name] = (EC.reference(c, np.float64), EC.reference(c, np.float32))
    return _REFS[name]


SMALL = tuple(n for n in EC.NAMES if EC.SPECS[n]["kind"] != "pack" and
              EC.SPECS[n].get("m", 0) * EC.SPECS[n].get("n", 0) * max(EC.SPECS[n]["batch"], 1) < 1 << 20)


@pytest.mark.parametrize("name", SMALL)
def test_reference_is_torch_double(name):
    c = case(name)
    ref, f32 = refs(name)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).double()
    if c["kind"] == "gemm":
        y = t(c["a"]) @ t(c["w"]).T
        if c["bias"] is not None:
            y = y + t(c["bias"])
        if c["flags"] & ER.SCALE:
            col = torch.arange(c["n"])
            col = col % c["scale_period"] if c["scale_period"] else col
            y = torch.where(col < c["scale_cols"], y * float(np.float32(c["scale"])), y)
        if c["flags"] & ER.GELU:
            y = torch.nn.functional.gelu(y)
        if c["flags"] & ER.RESIDUAL:
            y = y + t(c["r"])
    elif c["kind"] == "ln":
        y = torch.nn.functional.layer_norm(t(c["x"]), (c["d"],), t(c["gamma"]), t(c["beta"]), 1e-5)
    else:
        Z, T, d, H = c["qkv"].shape[0], c["T"], c["d"], c["H"]
        q, k, v = (t(c["qkv"][..., i * d:(i + 1) * d]).reshape(Z, T, H, 64).transpose(1, 2) for i in range(3))
        y = torch.nn.functional.scaled_dot_product_attention(q, k, v, scale=1.0).transpose(1, 2).reshape(Z, T, d)
    y = y.numpy()
    scale = np.maximum(1.0, np.abs(y))
    # (two double evaluations: scores of 300 carry 300 x 2^-52 each into the exponent, V values reach 60)
    assert np.max(np.abs(ref - y) / scale) < 1e-10, name
    # the restatement is inside its own tolerance, and is a float32 statement
    allowed, e32 = ER.value_tolerance(ref, f32)
    assert f32.dtype == np.float32 and np.all(ER.abs_err(f32, ref) <= allowed)
    assert e32 < 1e-3 * max(1.0, float(np.abs(ref).max())), (name, e32)


def test_equal_scores_give_the_mean_of_v():
    c = case("ax_t129_equal_b3")
    ref, _ = refs("ax_t129_equal_b3")
    mean = c["qkv"][..., 2 * c["d"]:].astype(np.float64).mean(axis=1, keepdims=True)
    assert np.max(np.abs(ref - mean)) < 1e-12


# ---- the format -------------------------------------------------------------------------------------------------------
def _bits(values):
    return np.array(values, np.uint32).view(np.float32)


def test_split_is_exact_on_its_domain_and_not_outside():
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 1 << 32, 400000, dtype=np.uint64).astype(np.uint32)
    bits = bits[(bits & 0x7F800000) != 0x7F800000]
    small = (rng.integers(0, 1 << 28, 200000, dtype=np.uint64).astype(np.uint32)) | (bits[:200000] & np.uint32(0x80000000))
    top = np.uint32(0x7F000000) + rng.integers(0, 0x7FFFFF + 1, 100000, dtype=np.uint64).astype(np.uint32)
    x = np.concatenate([bits.view(np.float32), small.view(np.float32), top.view(np.float32), EC.PACK_EDGE.view(np.float32),
                        rng.standard_normal(100000).astype(np.float32)])
    inside = ER.split_exact(x)
    planes = ER.split(x)
    value = ER.planes_value(planes)
    exact = value == x.astype(np.float64)
    assert inside.sum() > 500000 and (~inside).sum() > 10000
    assert np.all(exact[inside]), "hi + mid + lo != x inside the stated domain"
    # outside: every value at or above the overflow of hi is wrong (hi is infinite), and so is every value with bits under 2^-133
    assert not exact[~inside].any(), "the stated domain is too narrow: the split is exact on a value outside it"
    # the landmarks x3.h names
    for b, ok in ((0x7F7F7FFF, True), (0x7F7F8000, False), (0x7F7FFFFF, False), (0x00800000, True), (0x00800001, False),
                  (0x00000001, False), (0x00400000, True), (0x08800000, True), (0x08800001, True), (0x087FFFFF, False)):
        v = _bits([b])
        assert bool(ER.split_exact(v)[0]) == ok and bool(ER.planes_value(ER.split(v))[0] == float(v[0])) == ok, hex(b)
    assert float(_bits([0x08800000])[0]) == 2.0 ** -110      # from here on every float32 is a multiple of 2^-133


def test_row_image_round_trip_and_canonical_planes():
    rng = np.random.default_rng(6)
    x = rng.standard_normal((5, 72)).astype(np.float32) * np.float32(3.0)
    x[0, :2] = (-0.0, 0.0)                                                      # (- 0 is split as - 0, + 0, + 0)
    image = ER.pack_rows(x, 80)
    value, canonical = ER.decode_rows(image, 5, 72, 80)
    assert np.array_equal(value, x.astype(np.float64)) and canonical.all()
    # an image that sums to the same value but was split otherwise is not what a second X3 kernel expects
    other = image.copy()
    words = ER._row_words(5, 72, 80)
    hi = ER.bf16_value(other[words[2:3, 3]])[0]
    other[words[2, 3]] = ER.bf16_bits(hi * np.float32(0.5))[0]                    # hi halved, mid takes the other half
    other[words[2, 3] + 8] = ER.bf16_bits(hi * np.float32(0.5))[0]
    other[words[2, 3] + 16] = 0
    _, canonical = ER.decode_rows(other, 5, 72, 80)
    assert not canonical[2, 3] and canonical.sum() == canonical.size - 1
    own = ER.owned_words("rows", image.size, rows=5, cols=72, ld=80)
    assert own.sum() == 5 * 72 * 3 and not own.reshape(5, 240)[:, 216:].any()       # the pad chunk of every row is not owned


@pytest.mark.parametrize("T,d", [(33, 64), (64, 64), (70, 128), (97, 128)])
def test_attention_image_round_trip(T, d):
    rng = np.random.default_rng(T)
    qkv = rng.standard_normal((T, 3 * d)).astype(np.float32)
    image = ER.pack_attn_image(qkv)
    qk, v, canonical = ER.decode_attn_image(image, T, d)
    assert canonical and image.size == ER.attn_image_words(T, d)
    assert np.array_equal(qk, qkv[:, :2 * d].astype(np.float64)) and np.array_equal(v[:T], qkv[:, 2 * d:].astype(np.float64))
    assert not v[T:].any()
    assert ER.owned_words("qkv", image.size, T=T, d=d).all()         # the launch owns the whole image, pad keys included
    # the key order is ax_vt_key's: stored chunk u of a 32-key group holds keys 4u .. 4u + 3 and 16 + 4u .. 16 + 4u + 3
    order = ER.vt_key_order(32)
    assert order[:8].tolist() == [0, 1, 2, 3, 16, 17, 18, 19] and order[24:].tolist() == [12, 13, 14, 15, 28, 29, 30, 31]
    assert sorted(order.tolist()) == list(range(32))


# ---- coverage of the table ------------------------------------------------------------------------------------------------
def test_every_x3_flag_combination_of_the_encoder_is_a_case():
    """run_encode_group (csrc/api.hip) -> launch_gemm_x3: (flags, result form, table) of every launch"""
    S = EC.SPECS
    gemm = [s for s in S.values() if s["kind"] == "gemm"]

    def has(**kw):
        pred = kw.pop("pred", lambda s: True)
        return any(all(s[k] == v for k, v in kw.items()) and s["batch"] >= 1 and pred(s) for s in gemm)

    assert has(form=2, flags=ER.SCALE, pred=lambda s: s["scale_cols"] == 2 * s["d"] and not s["scale_period"])       # enc_qkv_x3 (image)
    assert has(form=0, flags=ER.RESIDUAL, r_is_c=True)                                                 # enc_out_x3, enc_fc2_x3
    assert has(form=1, flags=ER.GELU)                                                                              # enc_fc1_x3 (image)
    assert has(form=0, flags=ER.GELU)                                                                              # enc_fc1_x3 (fp32)
    assert has(form=0, flags=ER.SCALE, pred=lambda s: s["scale_period"] == 2 * s["scale_cols"] > 0)                 # dec_cross_kv_x3
    assert has(form=0, flags=ER.SCALE)                                                                             # enc_qkv_x3 (fp32) / cross kv
    for b in (0, 1, 2, 3, 8):
        assert any(s["batch"] == b for s in gemm), b
    for kind, forms in (("ln", (0,)), ("attention", (0, 1))):
        for form in forms:
            assert {s["batch"] for s in S.values() if s["kind"] == kind and s["form"] == form} >= {0, 1, 3, 8}, (kind, form)
    assert {s["m"] for s in gemm} >= set(EC.GEMM_M) and {s["n"] for s in gemm} >= set(EC.GEMM_N) | {1152, 2304}
    assert {s["k"] // 32 for s in gemm} >= {2, 4, 6, 10}
    for e in EC.EPILOGUES:
        assert any(n.endswith("_" + e) for n in EC.GEMM_NAMES), e


def test_walks_of_the_table():
    lib = _lib.load()
    seen = set()
    for name in EC.GEMM_NAMES:
        c = EC.SPECS[name]
        for walk in c["walks"]:
            p = EC.plan(lib, c, walk)
            assert int(p["bm"]) == walk[0] and int(p["persist"]) == walk[1] and ("colmajor" in p) == bool(walk[2]), (name, walk, p)
            assert int(p["nslab"]) == c["k"] // 32
            seen.add((int(p["bm"]), "banded" in p, "colmajor" in p, int(p["persist"])))
    for bm in (96, 64):
        for banded in (True, False):
            for colmajor in (True, False):
                for persist in (1, 0):
                    assert (bm, banded, colmajor, persist) in seen
    # the banded shape: nine 96-row tiles (the fourth row band is empty), thirteen 64-row tiles, nine tile columns
    p = EC.plan(lib, EC.SPECS["g_banded"], (96, 1, 1))
    assert p["tiles"] == "9x9" and "banded" in p and int(p["walked"]) == 81 < int(p["blocks"])       # workgroups without a tile
    assert EC.plan(lib, EC.SPECS["g_banded"], (64, 1, 1))["tiles"] == "13x9"
    # a workgroup that walks at least three tiles and skips an empty slot between two of them, at either height and order
    # (row-major is the order several sessions take by default; column-major, forced, still walks three tiles)
    for walk in ((96, 1, 0), (96, 1, 1), (64, 1, 0), (64, 1, 1)):
        p = EC.plan(lib, EC.SPECS["g_banded_b5_skip"], walk)
        assert int(p["max_tiles_per_wg"]) >= 3 and (walk[2] == 1 or p["skips_between"] == "1"), (walk, p)
    p = EC.plan(lib, EC.SPECS["g_banded_b5_skip"], (96, 0, 0))
    assert int(p["max_tiles_per_wg"]) == 1 and p["skips_between"] == "0"            # one workgroup per slot
    # plain walk with more tiles than workgroups
    p = EC.plan(lib, EC.SPECS["g_plain_b8_two_tiles"], (96, 1, 0))
    assert "plain" in p and int(p["max_tiles_per_wg"]) == 2 and int(p["blocks"]) == EC.CUS
    # the default geometry of the production shapes is what it was: base fc1, the N = d projection of a d = 1280 model alone
    # and with eight sessions
    for (m, n, k, batch), want in (((1500, 2048, 512, 1), dict(bm="96", colmajor="1", tiles="16x16", slots="32", blocks="256")),
                                   ((1500, 1280, 1280, 1), dict(bm="64", colmajor="1", tiles="24x10", slots="30", blocks="240")),
                                   ((1500, 1280, 1280, 8), dict(bm="96", rowmajor="1", tiles="16x10", slots="160", blocks="256"))):
        p = EC.plan(lib, dict(m=m, n=n, k=k, batch=batch), None)
        assert "banded" in p and p["persist"] == "1" and all(p.get(key) == val for key, val in want.items()), (m, n, k, batch, p)
    import ctypes
    buf = ctypes.create_string_buffer(320)
    assert lib.wlk_diag_x3_plan(8, 128, 96, 0, EC.CUS, buf, 320) == -1


def test_layernorm_and_attention_tables():
    S = EC.SPECS
    ln = [s for s in S.values() if s["kind"] == "ln"]
    npl = lambda d: next(n for n in (8, 12, 16, 20, 24) if (d + 63) // 64 <= n)
    assert {npl(s["d"]) for s in ln} == {8, 12, 16, 20, 24} and max(s["d"] for s in ln) == EC.LN_MAX_D == 1536
    assert any(s["d"] % 64 for s in ln) and {s["rows"] for s in ln} >= {1, 3, 4, 5}
    assert all(k in {kk for s in ln for kk in s["kinds"]} for k in EC.ROW_KINDS)
    ax = [s for s in S.values() if s["kind"] == "attention" and s["form"] == 1]
    tiles = {((s["T"] + 31) // 32) % 2 for s in ax}
    assert tiles == {0, 1}
    partial = {(((s["T"] + 31) // 32) - 1) % 2 for s in ax if s["T"] % 32}          # the stream that takes the partial last tile
    assert partial == {0, 1}
    assert any(s["T"] % 64 == 1 for s in ax)                                          # a last query tile of one row
    assert {s["T"] for s in ax} >= set(EC.AX_T) and {s["H"] for s in ax} == {1, 2, 3}
    for T in (65, 97):
        assert {s["inputs"] for s in ax if s["T"] == T} >= {"dominant_first", "dominant_last", "dominant_other"}
        assert EC.dominant_key(T, "dominant_other") // 32 == (T + 31) // 32 - 2
    pw = [s for s in S.values() if s["kind"] == "attention" and s["form"] == 0]
    assert {s["T"] for s in pw} >= {1, 31, 32, 33, 127, 128, 129}
    assert {s["inputs"] for s in ax} >= set(EC.ATT_KINDS)


# ---- deliberate mistakes ----------------------------------------------------------------------------------------------
MUTANT_CASES = {
    "residual_before_gelu": ("g_table_b8",),
    "scale_no_period": ("g_crosskv_d64", "g_table_b2"),
    "scale_boundary4": ("g_table_b2",),
    "bias_next_quad": ("g_table_b1",),
    "ln_unbiased": ("ln_d8", "ln_d384"),
    "ln_eps_outside": ("ln_d384",),
    "vt_plain_order": ("ax_t65_dominant_other", "ax_t64"),
    "drop_last_key": ("ax_t65_dominant_last", "pw_t129_dominant_last"),
    "pad_key_weight": ("ax_t129_equal_b3",),
    "softmax_no_max": ("ax_t97_offset300", "pw_t33_offset300"),
    "session0_operand": ("g_table_b3_alias", "ln_d384_r5_b8", "ax_t129_equal_b3"),
    "drop_lo": ("g_table_b1", "g_crosskv_d64"),
}


def test_mutant_table_is_complete():
    assert set(MUTANT_CASES) == set(ER.MUTANTS)


@pytest.mark.parametrize("mutant", ER.MUTANTS)
def test_deliberate_mistakes_are_caught(mutant):
    for name in MUTANT_CASES[mutant]:
        c = case(name)
        assert mutant in EC.mutants(c), (mutant, name)
        ref, f32 = refs(name)
        # (a softmax without the maximum is a float32 mistake: in double e^300 is still a number)
        wrong = EC.reference(c, np.float32 if mutant == "softmax_no_max" else np.float64, mutant)
        allowed, _ = ER.allowed_error(ref, f32, EC.family(c))
        assert (ER.abs_err(wrong, ref) > allowed).any(), f"{mutant} stays inside the tolerance of {name}"


def test_mistakes_on_every_case_they_bear_on():
    """beyond the named cases: a mistake changes most cases it bears on (counted, so that a table edit cannot hollow it out)"""
    caught = {m: [0, 0] for m in ER.MUTANTS}
    for name in SMALL:
        c = case(name)
        if c["kind"] == "gemm" and c["m"] * c["n"] > 40000:
            continue
        ref, f32 = refs(name)
        allowed, _ = ER.allowed_error(ref, f32, EC.family(c))
        for m in EC.mutants(c):
            wrong = EC.reference(c, np.float32 if m == "softmax_no_max" else np.float64, m)
            caught[m][1] += 1
            caught[m][0] += bool((ER.abs_err(wrong, ref) > allowed).any())
    for m, (hit, of) in caught.items():
        assert of > 0 and hit >= 1, (m, hit, of)
    # a two-plane product breaks the tolerance of most GEMM cases (not where a residual a thousand times the product, or a
    # saturated GELU, sets the scale of the output)
    assert 4 * caught["drop_lo"][0] >= 3 * caught["drop_lo"][1], caught["drop_lo"]
