"""What tests/test_gpu_linear.py and tests/test_gpu_gemm_tiles.py share: the buffers of one wlk_diag_linear_ex call as the
kernel sees them - every buffer with guard words (a NaN bit pattern) behind it, the rows of c n + 4 apart, c and the caches
arriving filled with the pattern - and the word checks on what came back.

A case (tests/linear_cases.py: build) may carry lda, any multiple of 4: above k the floats between two rows hold the
pattern, below k the rows overlap and the case's flat signal of (m - 1) lda + k floats is what lies in memory.  ldr is the
distance of the rows of r, whatever the distance of the rows of c.  The pattern follows the last addressed float of every
operand set; the sets of a batched call lie 4 floats (a: multiples of 4) or 7 floats (c, r) plus that apart."""
import ctypes as C

import numpy as np
import pytest

import linear_reference as LR
from whisperlivekit_amd import _lib

WLK_ERR_ARG = -1
GUARD = np.uint32(0x7FC12345)           # a NaN with a payload: reading it poisons, and it is recognisable
PAD = 4                                 # pad columns of the rows of c (and of r, unless the case names its ldr)
TAIL = 3                                # guard words behind every buffer


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
        k4 = (k + 3) // 4 * 4
        lda, ld = c.get("lda") or k4, n + PAD
        has_res, r_is_c = bool(c["flags"] & LR.RESIDUAL), c["r_is_c"]
        ldr = ld if r_is_c else (c.get("ldr") or ld)
        # floats from one operand set to the next: the last addressed float of a set, then 4 (7) guard words
        a_set, c_set, r_set = (m - 1) * lda + k4 + 4, m * ld + 7, m * ldr + 7
        self.a = guard(Z * a_set + TAIL)
        self.cbuf = guard(Z * c_set + TAIL)
        self.r = guard(Z * r_set + TAIL) if has_res and not r_is_c else None
        self.c_at = np.zeros((Z, m, n), np.int64)                             # float index of every output element
        for z in range(Z):
            if lda < k:                                                       # overlapping rows: the flat signal
                self.a[z * a_set:z * a_set + (m - 1) * lda + k] = c["a_flat"][z]
            else:
                self.a[z * a_set + np.arange(m)[:, None] * lda + np.arange(k)[None, :]] = c["a"][z]
            self.c_at[z] = z * c_set + np.arange(m)[:, None] * ld + np.arange(n)[None, :]
            if has_res and r_is_c:
                self.cbuf[self.c_at[z]] = c["r"][z]
            elif has_res:
                self.r[z * r_set + np.arange(m)[:, None] * ldr + np.arange(n)[None, :]] = c["r"][z]
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
                  kv_layer_off=c["kv_layer_off"], cache_stride=c["cache_stride"], lda=lda, ldr=ldr, ldc=ld,
                  a=self.a, a_floats=self.a.size, w=self.w, w_floats=self.w.size, bias=self.bias,
                  bias_floats=0 if self.bias is None else self.bias.size, ln_gamma=self.gamma, ln_beta=self.beta,
                  ln_floats=0 if self.gamma is None else self.gamma.size, r=self.r, r_floats=0 if self.r is None else self.r.size,
                  c=self.cbuf, c_floats=self.cbuf.size, kcache=self.kc, vcache=self.vc,
                  cache_floats=0 if self.kc is None else self.kc.size,
                  a_off=[z * a_set for z in range(Z)], c_off=[z * c_set for z in range(Z)], r_off=[z * r_set for z in range(Z)])
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
