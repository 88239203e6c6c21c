"""Named, seeded cases for the tiled fp32 GEMM kernels of csrc/gemm_f32.hip (tests/test_gpu_gemm_tiles.py) and their CPU
checks (tests/test_gemm_tile_cases_cpu.py): the smallest shapes at which each of the fifteen instantiations can still go
wrong - row and column tails, one live column in the last tile, the swizzled tile map with its padding workgroups and the
plain one, odd k-tile and slab counts, a last slab of four live columns, rows of a that overlap (lda < k: the conv stem)
or lie further apart than k, rows of r at another distance than the rows of c, operand tables.

A case is a spec of tests/linear_cases.py (same builder, same data kinds: a zero weight row, pre-activations over [-8, 8]
in front of an activation, one residual a thousand times the product, scale_cols off every multiple of 16) plus the kernel
every route was written for - PLAN[name][route], the text of wlk_diag_gemm_plan, which the CPU test holds against the
dispatch.  Routes are those of wlk_diag_linear_ex; TILE_ROUTES are the k-pipe kernel's eight tiles through launch_gemm_kp.
EPILOGUE[name] names the epilogue of a case; they rotate so that every instantiation meets every one of EPILOGUES."""
import linear_cases as LC
from linear_reference import GELU, RELU, RESIDUAL, SCALE, SWISH

SPECS = {}
PLAN = {}               # name -> {route: plan text}
EPILOGUE = {}           # name -> key of EPILOGUES
HEAD_OF = {}            # name -> (parent case, rows): the first rows of the parent, same weights, bias, epilogue and residual
TILES = ((3, 4), (3, 3), (3, 2), (3, 1), (2, 4), (2, 2), (2, 1), (4, 2))        # dispatch_kpipe's instantiations
TILE_ROUTES = tuple(500 + 10 * tm + tn for tm, tn in TILES)
INSTANTIATIONS = ("gemm<64,64>", "gemm<32,64>", "kwave<gemm>", "kwave16<gemm>", "kwave<kp,2>", "kwave<kp,1>", "kwave16<kp>") + \
    tuple(f"kpipe<{tm},{tn}>" for tm, tn in TILES)
EPILOGUES = ("gelu", "relu", "swish", "res", "res_c", "gelu_res", "scale", "period", "nobias")


def _off16(x):
    return x + 3 if x % 16 == 0 else x


def _epilogue(kind, n):
    period = max(5, n // 3)                                      # three periods and a tail
    return dict(gelu=dict(flags=GELU, spread=True), relu=dict(flags=RELU, spread=True), swish=dict(flags=SWISH, spread=True),
                res=dict(flags=RESIDUAL), res_c=dict(flags=RESIDUAL, r_is_c=True),
                gelu_res=dict(flags=GELU | RESIDUAL, spread=True), scale=dict(flags=SCALE, scale_cols=_off16(max(1, n // 3))),
                period=dict(flags=SCALE, scale_cols=_off16(max(1, period // 3)), scale_period=period),
                nobias=dict(bias=False))[kind]


_turn = [0]


def _add(name, m, n, k, plan, epilogue=None, **kw):
    """plan: {route: kernel}; the epilogue is the next of the rotation unless the case names it"""
    if epilogue is None:
        epilogue = EPILOGUES[_turn[0] % len(EPILOGUES)]
        _turn[0] += 1
    spec = dict(_epilogue(epilogue, n))
    spec.update(kw)
    LC._add(name, m, n, k, routes=tuple(plan), table=SPECS, **spec)
    PLAN[name], EPILOGUE[name] = dict(plan), epilogue


def _each(prefix, shapes, plan, epilogues=EPILOGUES):
    """every epilogue once, over the shapes in turn: (m, n, k) or (m, n, k, dict of further spec keys)"""
    for i, kind in enumerate(epilogues):
        m, n, k, *more = shapes[i % len(shapes)]
        kw = dict(more[0]) if more else {}
        lda = f"_lda{kw['lda']}" if kw.get("lda") else ""
        _add(f"{prefix}_{m}x{n}x{k}{lda}_{kind}", m, n, k, plan(m, n, k) if callable(plan) else plan, kind, **kw)


# ---- gemm<64,64>: route 3 and at least 64 tiles -------------------------------------------------------------------------
# 450 x 513: 8 x 9 tiles - the swizzled map with 8 padding workgroups, a 2-row and a 1-column tail; 200 x 1025: plain order,
# 3 k-tiles, so the pipeline's odd trip fetches past K; 512 x 512 x 4: one k-tile with four live columns
G64 = {3: "gemm<64,64>"}
_each("g64", ((450, 513, 36), (200, 1025, 68), (512, 512, 4)), G64, ("relu", "swish", "res_c", "scale", "period", "nobias"))
_add("g64_conv1_520x449_lda20_k60", 520, 449, 60, G64, "gelu", lda=20)                               # conv1 form
_add("g64_conv2_515x449_lda88_k132", 515, 449, 132, G64, "gelu_res", lda=88, ldr=449)                # conv2 form: ldr = n, ldc = n + 4
_add("g64_wide_lda_450x513x36", 450, 513, 36, G64, "res", lda=36 + 8, ldr=513 + 12, res_scale=1000.0)
_add("g64_conv1_batch3", 520, 449, 60, G64, "relu", lda=20, batch=3)                                 # operand table
_add("g64_route0_450x513x36", 450, 513, 36, {0: "gemm<64,64>", 3: "gemm<64,64>"}, "scale")

# ---- gemm<32,64>: route 3 and fewer than 64 tiles -----------------------------------------------------------------------
# 290 x 65: 10 tile rows - swizzled
G32 = {3: "gemm<32,64>"}
_each("g32", ((33, 65, 36), (290, 65, 132), (70, 120, 36, dict(lda=12))), G32)
_add("g32_route0_33x65x36", 33, 65, 36, {0: "gemm<32,64>", 3: "gemm<32,64>"}, "gelu_res")

# ---- kwave<gemm>: route 2 -----------------------------------------------------------------------------------------------
# 129 x 33 x 260: the last slab has 4 live columns; k = 384: an odd slab count
_each("kw", ((33, 70, 256), (129, 33, 260), (40, 120, 384), (40, 120, 384, dict(lda=128))), {2: "kwave<gemm>"})
_add("kw_route0_129x33x260", 129, 33, 260, {0: "kwave<gemm>", 2: "kwave<gemm>"}, "res")

# ---- kwave16<gemm>: route 0 with 9 <= m <= 128 (the two prefill-append shapes are cases of tests/linear_cases.py) ---------
_each("kw16", ((9, 17, 256), (17, 40, 260), (128, 40, 388)), {0: "kwave16<gemm>"})

# ---- the kp family's k-wave forms: routes 6, 7 and 8 (K % 128 == 0, M < 512), and route 5 where K is short ----------------
KP678 = {6: "kwave16<kp>", 7: "kwave<kp,2>", 8: "kwave<kp,1>"}
_each("kp", ((33, 70, 256), (300, 100, 384)), KP678, ("gelu", "relu", "swish", "res", "gelu_res"))
# K = 128 .. 255: k-wave tiles at every row count - 16 x 16 or 32 x 32 below 512 rows, 32 x 32 from there on
for _k, _kind in ((128, "res_c"), (160, "scale"), (192, "period"), (224, "nobias")):
    _add(f"kp_short_40x70x{_k}", 40, 70, _k, {5: "kwave16<kp>", **KP678}, _kind)
for _k, _kind in ((128, "gelu"), (160, "res"), (192, "res_c"), (224, "swish")):
    _add(f"kp_short_600x70x{_k}", 600, 70, _k, {5: "kwave<kp,2>", 6: "kwave<kp,2>", 7: "kwave<kp,2>", 8: "kwave<kp,1>"}, _kind)
# any other K: the plain tiled kernels, bit for bit route 3
_add("kp_other_70x120x36", 70, 120, 36, {3: "gemm<32,64>", 5: "gemm<32,64>"}, "swish")
_add("kp_other_130x65x320", 130, 65, 320, {3: "gemm<32,64>", 5: "gemm<32,64>"}, "res_c")
_add("kp_other_450x513x36", 450, 513, 36, {3: "gemm<64,64>", 5: "gemm<64,64>"}, "gelu")

# ---- kpipe<tm,tn>: every tile through route 500 + 10 tm + tn, route 4 (launch_gemm) and route 5 beside them ----------------
# 515 x 100 x 256: plain tile order for tm = 3 and 4, swizzled for tm = 2; N tails of 4, 36, 4 and 100 columns.
# 900 x 129 x 384: at least 8 tile rows for every tm, so padding workgroups everywhere; 1 live column in the last tile of
# tn = 1, 2 and 4, 33 for tn = 3.  Both take the 2 x 1 tile by ksplit_tile's and by kp_tile's choice.
KPIPE = {4: "kpipe<2,1>", 5: "kpipe<2,1>", **{r: f"kpipe<{tm},{tn}>" for r, (tm, tn) in zip(TILE_ROUTES, TILES)}}
_each("kpipe", ((515, 100, 256),), KPIPE, ("gelu", "relu", "scale", "nobias"))
_add("kpipe_515x100x256_res", 515, 100, 256, KPIPE, "res", ldr=100 + 8)
_each("kpipe", ((900, 129, 384),), KPIPE, ("swish", "res_c", "gelu_res", "period"))
# rows [0, 300) of the 900-row case on the k-wave forms: the family's promise - a row's bits do not depend on what is stacked under it
HEAD_OF["kp_head_300x129x384"] = ("kpipe_900x129x384_res_c", 300)
_add("kp_head_300x129x384", 300, 129, 384, KP678, "res_c")
# overlapped rows through a table (launch_gemm_kp takes no table: route 4 only)
_add("kpipe_batch2_515x128_lda256_k384", 515, 128, 384, {4: "kpipe<2,1>"}, "gelu_res", lda=256, batch=2)
# 512 rows and 1057 columns: ksplit_tile leaves 2 x 1 for 3 x 1, by shape too (K >= 512, N <= 1536: route 0)
_add("kpipe_own_512x1057x512", 512, 1057, 512, {0: "kpipe<3,1>", 4: "kpipe<3,1>"}, "res")

NAMES = tuple(SPECS)
REFUSED_SPECS = {}      # shapes only test_refusals builds
LC._add("x_tile_515x100x320", 515, 100, 320, table=REFUSED_SPECS)

# name -> (case, route, fragment of the refusal): tile routes wlk_diag_linear_ex refuses before anything is uploaded
REFUSALS = {
    "a tile the k-pipe kernel is not instantiated for": ("kpipe_515x100x256_relu", 555, "route in [0, 8]"),
    "a tile route with 300 rows": ("kp_300x100x384_relu", 534, "a k-pipe tile route needs a shape"),
    "a tile route with k = 320": ("x_tile_515x100x320", 521, "a k-pipe tile route needs a shape"),
}


def case(name):
    """-> the built case (tests/linear_cases.py: build), seeded by its name; a HEAD_OF case holds its parent's first rows"""
    if name not in HEAD_OF:
        return LC.build(name, SPECS[name] if name in SPECS else REFUSED_SPECS[name])
    parent, rows = HEAD_OF[name]
    p = LC.build(parent, SPECS[parent])
    s = SPECS[name]
    assert (s["n"], s["k"], s["flags"], s["r_is_c"], s["m"]) == (p["n"], p["k"], p["flags"], p["r_is_c"], rows) and not p["batch"]
    c = dict(p, name=name, m=rows, routes=s["routes"])
    c["a"] = p["a"][:, :rows]
    c["r"] = p["r"][:, :rows] if p["r"] is not None else None
    return c


def set_alone(c, z):
    """operand set z of batched case c as a case of its own"""
    s = dict(c, batch=0, name=f"{c['name']}[{z}]")
    s["a"] = c["a"][z:z + 1]
    s["a_flat"] = c["a_flat"][z:z + 1] if c["a_flat"] is not None else None
    s["r"] = c["r"][z:z + 1] if c["r"] is not None else None
    return s


def family(c, route):
    """the kernel family a route's outputs are judged as (linear_reference.OUTPUT_FACTOR is keyed by it): the kernel's name
    without its template arguments"""
    return PLAN[c["name"]][route].split("<")[0]
