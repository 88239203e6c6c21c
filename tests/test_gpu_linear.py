"""The linear layers of csrc/gemm_f32.hip - the single-row and the staged GEMV kernel in every instantiation launch_gemv
reaches, and the GEMM kernels' epilogue operands (scale_period, the prefill's cache append, operand tables) - one operator
per call through wlk_diag_linear_ex (production launchers, unchanged), against the float64 reference of
tests/linear_reference.py on the cases of tests/linear_cases.py.  No model, no session, no graph.

Tolerance (tests/select_reference.py: value_tolerance): a value may be off by 4 x the error the float32 restatement has on
the same case (floor 2^-22 * max(1, |reference|)); the GEMV kernels' fused LayerNorm has a measured factor of its own
(linear_reference.OUTPUT_FACTOR).  Every buffer has guard words - a NaN bit pattern - behind it, the rows
of c are n + 4 apart and c and the caches arrive filled with the pattern: what the reference does not write must still hold
it, every input must come back bit for bit, what goes to a cache is bit for bit what goes to c, a launch repeated gives the
same bits, and on route 1 every row of a call is bit for bit that row sent alone.  Every case writes its errors to
linear_report.json in the directory WLK_REPORT_DIR names (default: test_reports/)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import linear_cases as LC
import linear_reference as LR
from whisperlivekit_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}
WLK_ERR_ARG = -1
GUARD = np.uint32(0x7FC12345)           # a NaN with a payload: reading it poisons, and it is recognisable
PAD = 4                                 # pad columns of the rows of c and r
TAIL = 3                                # guard words behind every buffer


def report(key, value):
    REPORT[key] = value
    out = os.environ.get("WLK_REPORT_DIR") or os.path.join(ROOT, "test_reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "linear_report.json"), "w") as fh:
        json.dump(REPORT, fh, indent=1, sort_keys=True)


def guard(n):
    return np.full(n, GUARD, np.uint32).view(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def guarded(a):
    """`a` flattened into a buffer with TAIL guard words behind it"""
    a = np.ascontiguousarray(a, np.float32)
    buf = guard(a.size + TAIL)
    buf[:a.size] = a.reshape(-1)
    return buf


class Call:
    """the buffers of one wlk_diag_linear_ex call on case c, as the kernel sees them, and what came back"""

    def __init__(self, c, route, **override):
        m, n, k, Z = c["m"], c["n"], c["k"], max(c["batch"], 1)
        self.c, self.route = c, route
        lda, ld = (k + 3) // 4 * 4, n + PAD
        has_res, r_is_c = bool(c["flags"] & LR.RESIDUAL), c["r_is_c"]
        a_set, c_set = m * lda + 4, m * ld + 7                                # floats from one operand set to the next
        self.a = guard(Z * a_set + TAIL)
        self.cbuf = guard(Z * c_set + TAIL)
        self.r = guard(Z * c_set + TAIL) if has_res and not r_is_c else None
        self.c_at = np.zeros((Z, m, n), np.int64)                             # float index of every output element
        for z in range(Z):
            self.a[z * a_set:z * a_set + m * lda].reshape(m, lda)[:, :k] = c["a"][z]
            self.c_at[z] = z * c_set + np.arange(m)[:, None] * ld + np.arange(n)[None, :]
            if has_res:
                (self.cbuf if r_is_c else self.r)[self.c_at[z]] = c["r"][z]
        self.w = guarded(c["w"])
        self.bias = guarded(c["bias"]) if c["bias"] is not None else None
        self.gamma = guarded(c["gamma"]) if c["gamma"] is not None else None
        self.beta = guarded(c["beta"]) if c["beta"] is not None else None
        self.kc = guard(c["cache_floats"] + TAIL) if c["kv_mode"] else None
        self.vc = guard(c["cache_floats"] + TAIL) if c["kv_mode"] else None
        self.inputs = dict(a=self.a, w=self.w, bias=self.bias, gamma=self.gamma, beta=self.beta, r=self.r)
        self.sent = {key: None if v is None else v.copy() for key, v in
                     dict(self.inputs, c=self.cbuf, kc=self.kc, vc=self.vc).items()}
        kw = dict(route=route, m=m, n=n, k=k, flags=c["flags"], scale=float(c["scale"]), scale_cols=c["scale_cols"],
                  scale_period=c["scale_period"], r_is_c=int(r_is_c), kv_mode=c["kv_mode"], kv_pos=c["kv_pos"], kv_d=c["kv_d"],
                  kv_ctx=c["kv_ctx"], kv_ntok=c["kv_ntok"], n_caches=c["n_caches"], batch=c["batch"],
                  kv_layer_off=c["kv_layer_off"], cache_stride=c["cache_stride"], lda=lda, ldr=ld, ldc=ld,
                  a=self.a, a_floats=self.a.size, w=self.w, w_floats=self.w.size, bias=self.bias,
                  bias_floats=0 if self.bias is None else self.bias.size, ln_gamma=self.gamma, ln_beta=self.beta,
                  ln_floats=0 if self.gamma is None else self.gamma.size, r=self.r, r_floats=0 if self.r is None else self.r.size,
                  c=self.cbuf, c_floats=self.cbuf.size, kcache=self.kc, vcache=self.vc,
                  cache_floats=0 if self.kc is None else self.kc.size,
                  a_off=[z * a_set for z in range(Z)], c_off=[z * c_set for z in range(Z)], r_off=[z * c_set for z in range(Z)])
        if c["kv_rows"] is not None:
            kw.update(kv_row_cache=[r[0] for r in c["kv_rows"]], kv_row_offset=[r[1] for r in c["kv_rows"]])
        kw.update(override)
        args = _lib.DiagLinearArgs()
        for key, val in kw.items():
            if val is None:
                continue
            if isinstance(val, np.ndarray):
                assert val.flags["C_CONTIGUOUS"] and val.dtype == np.float32, key
                setattr(args, key, val.ctypes.data)
            elif isinstance(val, list):
                for i, x in enumerate(val):
                    getattr(args, key)[i] = int(x)
            else:
                setattr(args, key, val)
        lib = _lib.load()
        self.rc = lib.wlk_diag_linear_ex(C.byref(args))
        self.msg = "" if self.rc == 0 else lib.wlk_diag_last_error().decode()
        if self.rc not in (0, WLK_ERR_ARG):  # a HIP error: the device's state is unknown, nothing more is launched on it
            pytest.exit(f"wlk_diag_linear_ex ({c['name']}, route {route}): error {self.rc}: {self.msg}", returncode=3)
        self.out = self.cbuf[self.c_at]                                       # [Z][m][n]

    def changed(self, keys):
        return [key for key in keys if self.sent[key] is not None and
                not np.array_equal(bits(dict(self.inputs, c=self.cbuf, kc=self.kc, vc=self.vc)[key]), bits(self.sent[key]))]

    def check_words(self):
        """-> failures: inputs changed, words outside the outputs written, cache words that are not the values of c"""
        c, fails = self.c, []
        who = f"route {self.route}"
        changed = self.changed(self.inputs)
        if changed:
            fails.append(f"{who} changed its inputs: {changed}")
        outside = np.ones(self.cbuf.size, bool)
        outside[self.c_at.reshape(-1)] = False
        if not np.array_equal(bits(self.cbuf[outside]), bits(self.sent["c"][outside])):
            fails.append(f"{who} wrote outside the {c['m']} x {c['n']} outputs of c (pad columns, gaps or behind)")
        idx = LR.cache_indices(c)
        if idx is not None:
            d = c["kv_d"]
            for key, buf, cols in (("kcache", self.kc, slice(d, 2 * d)), ("vcache", self.vc, slice(2 * d, 3 * d))):
                rest = np.ones(buf.size, bool)
                rest[idx.reshape(-1)] = False
                if not np.all(bits(buf[rest]) == GUARD):
                    fails.append(f"{who} wrote {int((bits(buf[rest]) != GUARD).sum())} words of {key} the append does not own")
                if not np.array_equal(bits(buf[idx]), bits(self.out[0][:, cols])):
                    fails.append(f"{who}: {key} does not hold the bits that went to c "
                                 f"({int((bits(buf[idx]) != bits(self.out[0][:, cols])).sum())} words differ)")
        return fails


REFS = {}


def refs(c):
    """the float64 reference and the float32 restatement of a case, computed once"""
    if c["name"] not in REFS:
        REFS.clear()                    # (one case at a time: the largest is 2 x 8 x 32771 doubles)
        REFS[c["name"]] = (LR.linear(c, np.float64), LR.linear(c, np.float32))
    return REFS[c["name"]]


@pytest.mark.parametrize("name", LC.NAMES)
def test_linear(name):
    c = LC.case(name)
    ref, f32 = refs(c)
    failures, rep = [], {}
    for route in c["routes"]:
        tag = f"route{route}"
        first = Call(c, route)
        if first.rc != 0:
            failures.append(f"{tag}: error {first.rc}: {first.msg}")
            continue
        failures += first.check_words()
        entry, fail = LR.judge(tag, first.out, ref, f32, LC.family(c, route))
        rep[tag] = entry
        print(name, tag, json.dumps(entry))
        if fail:
            failures.append(fail)
        again = Call(c, route)
        if again.rc != 0 or not np.array_equal(bits(again.cbuf), bits(first.cbuf)) or (
                first.kc is not None and not (np.array_equal(bits(again.kc), bits(first.kc)) and
                                              np.array_equal(bits(again.vc), bits(first.vc)))):
            failures.append(f"{tag}: the same launch again gives other bits (rc {again.rc})")
        if route == 1 and (c["m"] > 1 or c["kv_mode"] == 2):
            # rows are independent and the single-row kernel is bit-identical to the staged one (csrc/gemm_f32.hip)
            for z in range(max(c["batch"], 1)):
                for row in range(c["m"]):
                    one = Call(LC.alone(c, z, row), 1)
                    if one.rc != 0:
                        failures.append(f"{tag}: row {row} alone: error {one.rc}: {one.msg}")
                    elif not np.array_equal(bits(one.out[0, 0]), bits(first.out[z, row])):
                        diff = bits(one.out[0, 0]) != bits(first.out[z, row])
                        failures.append(f"{tag}: row {row} differs from the same row alone in {int(diff.sum())} of {c['n']} features")
    report(name, rep)
    assert len(rep) == len(c["routes"]) and not failures, "\n".join(failures)


@pytest.mark.parametrize("what", list(LC.REFUSALS))
def test_refusals(what):
    base, override, route, fragment = LC.REFUSALS[what]
    call = Call(LC.case(base), override.get("route", route), **{k: v for k, v in override.items() if k != "route"})
    assert call.rc == WLK_ERR_ARG and fragment in call.msg, (what, call.rc, call.msg)
    assert not call.changed(["a", "w", "bias", "gamma", "beta", "r", "c", "kc", "vc"]), "a refused call touched a buffer"


def test_route_0_is_launch_linears_choice():
    """launch_linear by shape: the GEMV kernels up to 8 rows, the GEMM kernels from 9 on (512 x 120 x 256: the k-wave kernel) -
    the bits of the forced routes"""
    for name, forced in (("st_m8_n131_k2048", 1), ("gemm_period_kpipe", 2)):
        c = LC.case(name)
        a, b = Call(c, 0), Call(c, forced)
        assert a.rc == 0 and b.rc == 0, (a.msg, b.msg)
        assert np.array_equal(bits(a.cbuf), bits(b.cbuf)), name
