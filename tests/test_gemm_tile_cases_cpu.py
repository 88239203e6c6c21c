"""tests/gemm_tile_cases.py without a GPU: every (case, route) against the host dispatch (wlk_diag_gemm_plan - the answer
of the function launch_gemm and launch_gemm_kp launch), all fifteen instantiations and every epilogue on each of them; the
dispatch pinned at the production shapes, so that a moved threshold shows up as a diff of PINS; the float64 reference
against torch in double and the float32 restatement against the tolerance it defines; and the four mistakes of strides and
tails (linear_reference.MUTANTS) against that tolerance on every case they apply to."""
import ctypes as C

import numpy as np
import pytest

import gemm_tile_cases as GC
import linear_cases as LC
import linear_reference as LR
from test_linear_reference_cpu import torch_linear
from whisperlivekit_amd import _lib
from whisperlivekit_amd.dims import MODEL_DIMS

WLK_ERR_ARG = -1


def plan(m, n, k, route, batch=0, has_cache=0, buf=C.create_string_buffer(256)):
    rc = _lib.load().wlk_diag_gemm_plan(m, n, k, route, batch, has_cache, buf, len(buf))
    assert rc in (0, WLK_ERR_ARG)
    return rc, buf.value.decode()


# ---- plans ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GC.NAMES)
def test_every_route_of_a_case_reaches_the_kernel_it_was_written_for(name):
    s = GC.SPECS[name]
    assert set(GC.PLAN[name]) == set(s["routes"]) and s["lda"] % 4 == 0 and s["k"] % 4 == 0
    for route, kernel in GC.PLAN[name].items():
        assert plan(s["m"], s["n"], s["k"], route, s["batch"], int(s["kv_mode"] != 0)) == (0, kernel), (name, route)


def test_the_cases_cover_every_instantiation_with_every_epilogue():
    met = {}
    for name in GC.NAMES:
        for kernel in GC.PLAN[name].values():
            met.setdefault(kernel, set()).add(GC.EPILOGUE[name])
    assert set(met) == set(GC.INSTANTIATIONS) and len(GC.INSTANTIATIONS) == 15
    for kernel, kinds in met.items():
        assert kinds == set(GC.EPILOGUES), (kernel, sorted(set(GC.EPILOGUES) - kinds))


def test_the_table_holds_the_shapes_and_inputs_it_promises():
    S = GC.SPECS
    # scale_cols off every multiple of 16, a residual a thousand times the product, operand tables, strides of every kind
    assert all(s["scale_cols"] % 16 for s in S.values() if s["flags"] & LR.SCALE)
    assert any(s["res_scale"] == 1000.0 for s in S.values())
    c = GC.case("g64_wide_lda_450x513x36")
    assert np.median(np.abs(c["r"])) > 500 * np.median(np.abs(LR.linear(dict(c, flags=0), np.float64)))
    assert any(s["lda"] and s["lda"] < s["k"] and s["batch"] for s in S.values())
    assert any(s["lda"] > s["k"] for s in S.values())
    assert any(s["ldr"] == s["n"] for s in S.values()) and any(s["ldr"] > s["n"] + LC.PAD for s in S.values())
    for name in GC.NAMES:
        c = GC.case(name)
        assert not c["w"][c["n"] // 2].any(), name
        if c["lda"] and c["lda"] < c["k"]:          # the rows are a view of the signal, not copies
            assert c["a_flat"].shape == (max(c["batch"], 1), (c["m"] - 1) * c["lda"] + c["k"])
            assert np.array_equal(c["a"][0, 1], c["a_flat"][0, c["lda"]:c["lda"] + c["k"]])
    # k-pipe tile shapes: both tile orders and a padded map for every tile, one live column in a last tile
    for tm, tn in GC.TILES:
        assert (900 + 32 * tm - 1) // (32 * tm) >= 8
    assert {(515 + 32 * tm - 1) // (32 * tm) >= 8 for tm, _ in GC.TILES} == {True, False}
    assert {129 % (32 * tn) for _, tn in GC.TILES} == {1, 33}
    head, (parent, rows) = GC.case("kp_head_300x129x384"), GC.HEAD_OF["kp_head_300x129x384"]
    p = GC.case(parent)
    assert np.array_equal(head["a"], p["a"][:, :rows]) and np.array_equal(head["r"], p["r"][:, :rows]) and head["w"] is not p["w"]
    assert np.array_equal(head["w"], p["w"]) and np.array_equal(head["bias"], p["bias"])


def test_every_own_choice_has_a_forced_route_beside_it():
    """tests/test_gpu_gemm_tiles.py compares routes 0 and 5 with the forced route of the same kernel: no route 0 / 5 of the table
    is without one, except kwave16<gemm>, which only
    launch_gemm's own choice reaches"""
    for name in GC.NAMES:
        p = GC.PLAN[name]
        for own in (0, 5):
            if own in p and p[own] != "kwave16<gemm>":
                assert any(k == p[own] for r, k in p.items() if r not in (0, 5)), (name, own)


def test_plan_refusals():
    for args, fragment in (((515, 100, 256, 555), "route in [0, 8]"), ((515, 100, 256, 9), "route in [0, 8]"),
                           ((300, 100, 384, 534), "a k-pipe tile route needs a shape"),
                           ((515, 100, 320, 521), "a k-pipe tile route needs a shape"),
                           ((8, 100, 256, 0), "launch_gemv"), ((40, 100, 256, 1), "launch_gemv"),
                           ((40, 100, 254, 3), "multiples of 4"), ((300, 100, 256, 4), "does not take this shape"),
                           ((40, 120, 256, 6, 2), "plain projections only"), ((40, 120, 256, 2, 2), "batched launches"),
                           ((14, 120, 36, 0, 0, 1), "only available on the k-wave path"), ((0, 100, 256, 3), "m >= 1")):
        rc, text = plan(*args)
        assert rc == WLK_ERR_ARG and fragment in text, (args, rc, text)


# ---- dispatch pins ----------------------------------------------------------------------------------------------------
def production_shapes():
    """label -> (route, m, n, k, has_cache): what the models send to launch_gemm (route 0) and launch_gemm_kp (route 5)"""
    out = {}
    for d, mels in sorted({(x.n_audio_state, x.n_mels) for x in MODEL_DIMS.values()}):
        out[f"whisper d={d} mels={mels} conv1 m=3000"] = (0, 3000, d, 3 * mels, 0)
    for d in sorted({x.n_audio_state for x in MODEL_DIMS.values()}):
        for what, n, k in (("conv2", d, 3 * d), ("qkv", 3 * d, d), ("out", d, d), ("fc1", 4 * d, d), ("fc2", d, 4 * d)):
            out[f"whisper d={d} {what} m=1500"] = (0, 1500, n, k, 0)
            if what != "conv2":
                out[f"whisper d={d} {what} m=3000"] = (0, 3000, n, k, 0)           # two stacked encodes
                for rows in (9, 60, 128, 129, 448):                                # decoder prefill (-1: see shape_plan)
                    out[f"whisper d={d} {what} prefill m={rows}"] = (0, rows, n, k, -1 if what == "qkv" else 0)
    d, ff, dt, inner = 512, 2048, 192, 768                                         # Sortformer: every projection is kp
    for m in (50, 401, 802, 3208):
        for what, n, k in (("ff in", ff, d), ("ff out", d, ff), ("qkv", 3 * d, d), ("att out", d, d), ("pw1", 2 * d, d),
                           ("proj", dt, d), ("tf qkv", 3 * dt, dt), ("tf out", dt, dt), ("tf in", inner, dt), ("tf outd", dt, inner)):
            out[f"sortformer {what} m={m}"] = (5, m, n, k, 0)
    d = 1024                                                                       # NLLB encoders (600M: ffn 4096, 1.3B: 8192)
    for m in (16, 128, 512):
        for what, n, k in (("qkv", 3 * d, d), ("out", d, d), ("xkv", 2 * d, d), ("fc1 4096", 4096, d), ("fc2 4096", d, 4096),
                           ("fc1 8192", 8192, d), ("fc2 8192", d, 8192)):
            out[f"nllb {what} m={m}"] = (0, m, n, k, 0)
    return out


def shape_plan(route, m, n, k, cache):
    """has_cache -1: the prefill's q | k | v appends to the caches in the same launch where the k-wave kernels take the shape
    (api.hip asks gemm_takes_kwave), and is a plain projection elsewhere"""
    rc, text = plan(m, n, k, route, 0, max(cache, 0))
    if cache == -1 and rc == 0 and text.startswith("kwave"):
        rc, text = plan(m, n, k, route, 0, 1)
    return rc, text


# plan -> labels, written from wlk_diag_gemm_plan's answers: a change of dispatch is a diff of this table
PINS = {
    "gemm<32,64>": (
        "whisper d=128 qkv prefill m=9", "whisper d=128 qkv prefill m=60", "whisper d=128 qkv prefill m=128",
        "whisper d=128 qkv prefill m=129", "whisper d=128 qkv prefill m=448", "whisper d=128 out m=1500",
        "whisper d=128 out prefill m=9", "whisper d=128 out prefill m=60", "whisper d=128 out prefill m=128",
        "whisper d=128 out prefill m=129", "whisper d=128 out prefill m=448", "whisper d=128 fc1 prefill m=9",
        "whisper d=128 fc1 prefill m=60", "whisper d=128 fc1 prefill m=128", "whisper d=128 fc1 prefill m=129",
        "whisper d=128 fc1 prefill m=448",
    ),
    "gemm<64,64>": (
        "whisper d=128 mels=80 conv1 m=3000", "whisper d=384 mels=80 conv1 m=3000", "whisper d=512 mels=80 conv1 m=3000",
        "whisper d=768 mels=80 conv1 m=3000", "whisper d=1024 mels=80 conv1 m=3000", "whisper d=1280 mels=80 conv1 m=3000",
        "whisper d=1280 mels=128 conv1 m=3000", "whisper d=128 qkv m=1500", "whisper d=128 qkv m=3000",
        "whisper d=128 out m=3000", "whisper d=128 fc1 m=1500", "whisper d=128 fc1 m=3000", "whisper d=384 qkv m=1500",
        "whisper d=384 qkv m=3000", "whisper d=384 qkv prefill m=448", "whisper d=384 out m=1500",
        "whisper d=384 out m=3000", "whisper d=384 fc1 m=1500", "whisper d=384 fc1 m=3000",
        "whisper d=384 fc1 prefill m=448", "whisper d=512 qkv prefill m=448", "whisper d=512 fc1 m=1500",
        "whisper d=512 fc1 m=3000", "whisper d=512 fc1 prefill m=448", "whisper d=768 qkv m=1500",
        "whisper d=768 qkv m=3000", "whisper d=768 qkv prefill m=448", "whisper d=768 fc1 m=1500",
        "whisper d=768 fc1 m=3000", "whisper d=768 fc1 prefill m=129", "whisper d=768 fc1 prefill m=448",
        "whisper d=1024 qkv m=1500", "whisper d=1024 qkv m=3000", "whisper d=1024 qkv prefill m=129",
        "whisper d=1024 qkv prefill m=448", "whisper d=1024 out prefill m=448", "whisper d=1024 fc1 m=1500",
        "whisper d=1024 fc1 m=3000", "whisper d=1024 fc1 prefill m=128", "whisper d=1024 fc1 prefill m=129",
        "whisper d=1024 fc1 prefill m=448", "whisper d=1024 fc2 prefill m=448", "whisper d=1280 qkv m=1500",
        "whisper d=1280 qkv m=3000", "whisper d=1280 qkv prefill m=128", "whisper d=1280 qkv prefill m=129",
        "whisper d=1280 qkv prefill m=448", "whisper d=1280 out prefill m=448", "whisper d=1280 fc1 m=1500",
        "whisper d=1280 fc1 m=3000", "whisper d=1280 fc1 prefill m=128", "whisper d=1280 fc1 prefill m=129",
        "whisper d=1280 fc1 prefill m=448", "whisper d=1280 fc2 prefill m=448", "nllb fc1 4096 m=128",
        "nllb fc1 8192 m=128", "nllb qkv m=512", "nllb xkv m=512", "nllb fc1 4096 m=512", "nllb fc1 8192 m=512",
    ),
    "kpipe<2,1>": (
        "whisper d=128 fc2 m=1500", "whisper d=128 fc2 m=3000", "sortformer ff out m=802", "sortformer att out m=802",
        "sortformer proj m=802", "sortformer tf outd m=802", "sortformer ff in m=3208", "sortformer pw1 m=3208",
        "nllb out m=512", "nllb fc2 4096 m=512", "nllb fc2 8192 m=512",
    ),
    "kpipe<2,2>": (
        "sortformer qkv m=3208",
    ),
    "kpipe<2,4>": (
        "whisper d=1280 conv2 m=1500", "whisper d=1280 out m=1500", "whisper d=1280 out m=3000",
        "whisper d=1280 fc2 m=1500", "whisper d=1280 fc2 m=3000", "sortformer ff out m=3208", "sortformer att out m=3208",
    ),
    "kpipe<3,1>": (
        "whisper d=384 conv2 m=1500", "whisper d=384 fc2 m=1500", "whisper d=512 conv2 m=1500", "whisper d=512 out m=1500",
        "whisper d=512 fc2 m=1500", "sortformer pw1 m=802", "sortformer proj m=3208", "sortformer tf outd m=3208",
    ),
    "kpipe<3,2>": (
        "whisper d=384 fc2 m=3000", "whisper d=512 out m=3000", "whisper d=512 fc2 m=3000", "whisper d=768 conv2 m=1500",
        "whisper d=768 out m=1500", "whisper d=768 fc2 m=1500", "whisper d=1024 conv2 m=1500", "whisper d=1024 out m=1500",
        "whisper d=1024 fc2 m=1500", "sortformer ff in m=802", "sortformer qkv m=802",
    ),
    "kpipe<3,3>": (
        "whisper d=512 qkv m=1500", "whisper d=512 qkv m=3000", "whisper d=768 out m=3000", "whisper d=768 fc2 m=3000",
    ),
    "kpipe<3,4>": (
        "whisper d=1024 out m=3000", "whisper d=1024 fc2 m=3000",
    ),
    "kwave16<gemm>": (
        "whisper d=128 fc2 prefill m=9", "whisper d=128 fc2 prefill m=60", "whisper d=128 fc2 prefill m=128",
        "whisper d=384 qkv prefill m=9", "whisper d=384 qkv prefill m=60", "whisper d=384 qkv prefill m=128",
        "whisper d=384 out prefill m=9", "whisper d=384 out prefill m=60", "whisper d=384 out prefill m=128",
        "whisper d=384 fc1 prefill m=9", "whisper d=384 fc1 prefill m=60", "whisper d=384 fc1 prefill m=128",
        "whisper d=384 fc2 prefill m=9", "whisper d=384 fc2 prefill m=60", "whisper d=384 fc2 prefill m=128",
        "whisper d=512 qkv prefill m=9", "whisper d=512 qkv prefill m=60", "whisper d=512 qkv prefill m=128",
        "whisper d=512 out prefill m=9", "whisper d=512 out prefill m=60", "whisper d=512 out prefill m=128",
        "whisper d=512 fc1 prefill m=9", "whisper d=512 fc1 prefill m=60", "whisper d=512 fc1 prefill m=128",
        "whisper d=512 fc2 prefill m=9", "whisper d=512 fc2 prefill m=60", "whisper d=512 fc2 prefill m=128",
        "whisper d=768 qkv prefill m=9", "whisper d=768 qkv prefill m=60", "whisper d=768 qkv prefill m=128",
        "whisper d=768 out prefill m=9", "whisper d=768 out prefill m=60", "whisper d=768 out prefill m=128",
        "whisper d=768 fc1 prefill m=9", "whisper d=768 fc1 prefill m=60", "whisper d=768 fc1 prefill m=128",
        "whisper d=768 fc2 prefill m=9", "whisper d=768 fc2 prefill m=60", "whisper d=768 fc2 prefill m=128",
        "whisper d=1024 qkv prefill m=9", "whisper d=1024 qkv prefill m=60", "whisper d=1024 qkv prefill m=128",
        "whisper d=1024 out prefill m=9", "whisper d=1024 out prefill m=60", "whisper d=1024 out prefill m=128",
        "whisper d=1024 fc1 prefill m=9", "whisper d=1024 fc1 prefill m=60", "whisper d=1024 fc2 prefill m=9",
        "whisper d=1024 fc2 prefill m=60", "whisper d=1024 fc2 prefill m=128", "whisper d=1280 qkv prefill m=9",
        "whisper d=1280 qkv prefill m=60", "whisper d=1280 out prefill m=9", "whisper d=1280 out prefill m=60",
        "whisper d=1280 out prefill m=128", "whisper d=1280 fc1 prefill m=9", "whisper d=1280 fc1 prefill m=60",
        "whisper d=1280 fc2 prefill m=9", "whisper d=1280 fc2 prefill m=60", "whisper d=1280 fc2 prefill m=128",
        "nllb qkv m=16", "nllb out m=16", "nllb xkv m=16", "nllb fc1 4096 m=16", "nllb fc2 4096 m=16", "nllb fc1 8192 m=16",
        "nllb fc2 8192 m=16", "nllb qkv m=128", "nllb out m=128", "nllb xkv m=128", "nllb fc2 4096 m=128",
        "nllb fc2 8192 m=128",
    ),
    "kwave16<kp>": (
        "sortformer ff in m=50", "sortformer ff out m=50", "sortformer qkv m=50", "sortformer att out m=50",
        "sortformer pw1 m=50", "sortformer proj m=50", "sortformer tf qkv m=50", "sortformer tf out m=50",
        "sortformer tf in m=50", "sortformer tf outd m=50", "sortformer att out m=401", "sortformer proj m=401",
        "sortformer tf qkv m=401", "sortformer tf out m=401", "sortformer tf in m=401", "sortformer tf outd m=401",
    ),
    "kwave<gemm>": (
        "whisper d=128 conv2 m=1500", "whisper d=128 fc2 prefill m=129", "whisper d=128 fc2 prefill m=448",
        "whisper d=384 qkv prefill m=129", "whisper d=384 out prefill m=129", "whisper d=384 out prefill m=448",
        "whisper d=384 fc1 prefill m=129", "whisper d=384 fc2 prefill m=129", "whisper d=384 fc2 prefill m=448",
        "whisper d=512 qkv prefill m=129", "whisper d=512 out prefill m=129", "whisper d=512 out prefill m=448",
        "whisper d=512 fc1 prefill m=129", "whisper d=512 fc2 prefill m=129", "whisper d=512 fc2 prefill m=448",
        "whisper d=768 qkv prefill m=129", "whisper d=768 out prefill m=129", "whisper d=768 out prefill m=448",
        "whisper d=768 fc2 prefill m=129", "whisper d=768 fc2 prefill m=448", "whisper d=1024 out prefill m=129",
        "whisper d=1024 fc2 prefill m=129", "whisper d=1280 out prefill m=129", "whisper d=1280 fc2 prefill m=129",
    ),
    "kwave<kp,1>": (
        "sortformer ff in m=401", "sortformer qkv m=401", "sortformer tf in m=802", "sortformer tf qkv m=3208",
        "sortformer tf out m=3208", "sortformer tf in m=3208",
    ),
    "kwave<kp,2>": (
        "sortformer ff out m=401", "sortformer pw1 m=401", "sortformer tf qkv m=802", "sortformer tf out m=802",
    ),
}


def test_dispatch_pins():
    shapes = production_shapes()
    now = {}
    for label, (route, m, n, k, cache) in shapes.items():
        rc, text = shape_plan(route, m, n, k, cache)
        assert rc == 0, (label, text)
        now.setdefault(text, []).append(label)
    pinned = {label: kernel for kernel, labels in PINS.items() for label in labels}
    assert sum(len(v) for v in PINS.values()) == len(pinned) and set(pinned) == set(shapes)
    moved = {label: (pinned[label], kernel) for kernel, labels in now.items() for label in labels if pinned[label] != kernel}
    assert not moved, f"shapes that changed their kernel (pinned, now): {moved}"
    covered = {kernel for name in GC.NAMES for kernel in GC.PLAN[name].values()}
    assert set(PINS) <= covered, sorted(set(PINS) - covered)


# ---- reference, restatement, mutants ----------------------------------------------------------------------------------
NEW_MUTANTS = ("lda_is_k", "ldr_is_ldc", "k_tail_dropped", "tail_row_clamped")


@pytest.mark.parametrize("name", GC.NAMES)
def test_reference_restatement_and_mutants(name):
    c = GC.case(name)
    ref, f32 = LR.linear(c, np.float64), LR.linear(c, np.float32)
    assert ref.dtype == np.float64 and f32.dtype == np.float32 and ref.shape == (max(c["batch"], 1), c["m"], c["n"])
    assert np.all(np.isfinite(ref))
    assert np.abs(ref - torch_linear(c)).max() <= 1e-11 * max(1.0, np.abs(ref).max())
    entry, fail = LR.judge("restatement", f32, ref, f32)
    assert fail is None and np.isfinite(entry["restatement_err"]), (entry, fail)
    assert {GC.family(c, r) for r in c["routes"]} <= {"gemm", "kwave", "kwave16", "kpipe"} and not set(LR.OUTPUT_FACTOR) & {
        "gemm", "kwave", "kwave16", "kpipe"}
    allowed = LR.allowed_error(ref, f32)[0]
    for mutant in LC.mutants(c):
        if mutant in NEW_MUTANTS:           # every case a mistake applies to tells it from the reference, by a wide margin
            err = LR.abs_err(LR.linear(c, np.float64, mutant), ref)
            assert (err > 8 * allowed).any(), f"{name} does not tell {mutant} from the reference"


def test_every_new_mutant_applies_somewhere():
    for mutant in NEW_MUTANTS:
        assert mutant in LR.MUTANTS
        assert any(mutant in LC.mutants(GC.SPECS[n]) for n in GC.NAMES), mutant
