"""The encoder's production kernel routes - the X3 GEMM (csrc/gemm_x3.hip) with every epilogue operand, result form, walk
and operand table run_encode_group launches, the LayerNorm kernels, the fp32 and the X3 self-attention - one operator per
call through wlk_diag_enc_op (production launchers, unchanged), against the float64 reference of
tests/enc_x3_reference.py on the cases of tests/enc_x3_cases.py.  No model, no session, no graph.

Tolerance (tests/select_reference.py: value_tolerance): a value may be off by 4 x the error the float32 restatement has on
the same case (floor 2^-22 * max(1, |reference|)); a family with a measured factor of its own is named in
enc_x3_reference.OUTPUT_FACTOR.  X3 results come back as raw 16-bit words and are decoded here, not by the device.  Every
buffer has guard words - a NaN bit pattern - behind it, between its operand sets and in its pad columns, and results arrive
filled with the pattern: what a result form does not own must still hold it, what it owns must all have lost it, every input
must come back bit for bit.  Bit identities the kernels' comments promise are asserted as such.  Every case writes its
figures to enc_x3_report.json in the directory WLK_REPORT_DIR names (default: test_reports/)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import enc_x3_cases as EC
import enc_x3_reference as ER
from whisperlivekit_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}
WLK_ERR_ARG = -1
GUARD = np.uint32(0x7FC12345)           # a NaN with a payload: reading it poisons, and it is recognisable
GUARD16 = np.uint16(0x7FC1)             # the same for a bf16 plane word
TAIL = 3                                # guard words behind every buffer
POINTERS = ("in", "in3", "w", "bias", "r", "out", "out3")
SIZES = dict(zip(POINTERS, ("in_floats", "in3_elems", "w_floats", "bias_floats", "r_floats", "out_floats", "out3_elems")))


def report(key, value):
    REPORT[key] = value
    out = os.environ.get("WLK_REPORT_DIR") or os.path.join(ROOT, "test_reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "enc_x3_report.json"), "w") as fh:
        json.dump(REPORT, fh, indent=1, sort_keys=True)


def guard(n):
    return np.full(n, GUARD, np.uint32).view(np.float32)


def guard16(n):
    return np.full(n, GUARD16, np.uint16)


def bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype == np.uint16 else a.astype(np.float32, copy=False).view(np.uint32)


def guarded(a):
    a = np.ascontiguousarray(a, np.float32)
    buf = guard(a.size + TAIL)
    buf[:a.size] = a.reshape(-1)
    return buf


def offsets(set_words, Z, step):
    """-> (offset of every operand set, total words): set z is followed by a gap of step * (z + 1) guard words"""
    off, at = [], 0
    for z in range(Z):
        off.append(at)
        at += set_words + step * (z + 1)
    return off, at + TAIL


class Op:
    """one wlk_diag_enc_op call: numpy buffers for the pointer fields, everything else as given; keeps what was sent"""

    def __init__(self, who, walk=None, **kw):
        self.buf = {key: kw.pop(key, None) for key in POINTERS}
        self.sent = {key: None if v is None else v.copy() for key, v in self.buf.items()}
        args = _lib.DiagEncOpArgs()
        for key, v in self.buf.items():
            if v is not None:
                assert v.flags["C_CONTIGUOUS"] and v.dtype == (np.uint16 if key.endswith("3") else np.float32), key
                setattr(args, key, v.ctypes.data)
                setattr(args, SIZES[key], v.size)
        for key, val in kw.items():
            if isinstance(val, (list, tuple)):
                for i, x in enumerate(val):
                    getattr(args, key)[i] = int(x)
            else:
                setattr(args, key, val)
        lib = _lib.load()
        old = {key: os.environ.get(key) for key in EC.ENV_KEYS}
        try:
            if walk is not None:
                for key, val in zip(EC.ENV_KEYS, walk):
                    os.environ[key] = str(val)
                lib.wlk_diag_env_refresh()
            self.rc = lib.wlk_diag_enc_op(C.byref(args))
        finally:
            for key, val in old.items():
                if val is None:
                    os.environ.pop(key, None)
                else:
                    os.environ[key] = val
            lib.wlk_diag_env_refresh()
        self.msg = "" if self.rc == 0 else lib.wlk_diag_last_error().decode()
        if self.rc not in (0, WLK_ERR_ARG):     # a HIP error: the device's state is unknown, nothing more is launched on it
            pytest.exit(f"wlk_diag_enc_op ({who}): error {self.rc}: {self.msg}", returncode=3)

    def changed(self, keys=POINTERS):
        return [key for key in keys if self.sent[key] is not None and not np.array_equal(bits(self.buf[key]), bits(self.sent[key]))]

    def check_words(self, who, results, may_keep=None):
        """results: {pointer: bool mask of the words the launch owns}.  -> failures: an input changed, a word outside the
        result written, an owned word that still holds what arrived - the guard, or with r_is_c the residual; may_keep
        masks the words of a preloaded result whose new value may be the old one"""
        fails = []
        changed = self.changed([k for k in POINTERS if k not in results])
        if changed:
            fails.append(f"{who} changed its inputs: {changed}")
        for key, own in results.items():
            now, sent = bits(self.buf[key]), bits(self.sent[key])
            if not np.array_equal(now[~own], sent[~own]):
                fails.append(f"{who} wrote {int((now[~own] != sent[~own]).sum())} words of {key} it does not own (pad columns, gaps or behind)")
            kept = own & (now == sent)
            if may_keep is not None:
                kept &= ~may_keep
            if kept.any():
                fails.append(f"{who} left {int(kept.sum())} owned words of {key} unwritten (first at {int(np.argmax(kept))})")
        return fails


# ----------------------------------------------------------------------------------------------------------------------
# builders: case -> Op, and where its outputs lie
# ----------------------------------------------------------------------------------------------------------------------
class Gemm:
    def __init__(self, c, walk=None, form=None, **override):
        form = c["form"] if form is None else form
        batch = c["batch"]
        Z, m, n, k = max(batch, 1), c["m"], c["n"], c["k"]
        self.c, self.form, self.Z = c, form, Z
        lda, ld = k + 8, n + 4
        has_res, r_is_c = bool(c["flags"] & ER.RESIDUAL), c["r_is_c"]
        a_off, a_size = offsets(m * lda, Z, 4)
        a = guard(a_size)
        for z in range(Z):
            a[a_off[z]:a_off[z] + m * lda].reshape(m, lda)[:, :k] = c["a"][z]
        kw = dict(kind=_lib.ENC_X3_GEMM, form=form, m=m, n=n, k=k, flags=c["flags"], scale=float(c["scale"]),
                  scale_cols=c["scale_cols"], scale_period=c["scale_period"], r_is_c=int(r_is_c), batch=batch, ld_in=lda,
                  in_off=a_off, w=guarded(c["w"]), bias=None if c["bias"] is None else guarded(c["bias"]))
        kw["in"] = a
        if form == 0:
            c_off, c_size = offsets(m * ld, Z, 4)
            out = guard(c_size)
            self.at = np.stack([c_off[z] + np.arange(m)[:, None] * ld + np.arange(n)[None, :] for z in range(Z)])
            self.own = np.zeros(c_size, bool)
            self.own[self.at.reshape(-1)] = True
            if has_res and r_is_c:
                out[self.at] = c["r"][:Z]
            elif has_res:
                r = guard(c_size)
                r[self.at] = c["r"][:Z]
                kw.update(r=r, ldr=ld, r_off=c_off)
            kw.update(out=out, ld_out=ld, out_off=c_off)
            self.key = "out"
        else:
            if form == 1:
                ld3 = (n + 7) // 8 * 8 + 8
                words = m * 3 * ld3
                kw.update(vt_col0=(n + 127) // 128 * 128, vt_off=0, vt_ld=ER.vt_ld(m))      # (fc1: vt_col0 = n, a multiple of 128)
            else:
                d = c["d"]
                ld3, words = 2 * d, ER.attn_image_words(m, d)
                kw.update(vt_col0=2 * d, vt_off=ER.vt_off(m, d), vt_ld=ER.vt_ld(m))
            self.off3, size = offsets(words, Z, 8)
            self.words = words
            self.own = np.zeros(size, bool)
            for z in range(Z):
                self.own |= (ER.owned_words("rows", size, rows=m, cols=n, ld=ld3, at=self.off3[z]) if form == 1 else
                             ER.owned_words("qkv", size, T=m, d=c["d"], at=self.off3[z]))
            kw.update(out3=guard16(size), ld_out3=ld3, out3_off=self.off3)
            self.ld3 = ld3
            self.key = "out3"
        kw.update(override)
        self.op = Op(c["name"], walk, **kw)
        self.rc, self.msg = self.op.rc, self.op.msg

    @property
    def result(self):
        return self.op.buf[self.key]

    def values(self):
        """-> (float64 [Z][m][n], canonical): the result as values; an X3 result is decoded here"""
        c, m, n = self.c, self.c["m"], self.c["n"]
        if self.form == 0:
            return self.result[self.at].astype(np.float64), True
        out, ok = np.empty((self.Z, m, n)), True
        for z in range(self.Z):
            img = self.result[self.off3[z]:]
            if self.form == 1:
                out[z], can = ER.decode_rows(img, m, n, self.ld3)
                ok = ok and bool(can.all())
            else:
                qk, v, can = ER.decode_attn_image(img, m, c["d"])
                out[z] = np.concatenate([qk, v[:m]], axis=1)
                ok = ok and can and not v[m:].any() and not np.signbit(v[m:]).any()       # the pad keys are + 0
        return out, ok

    def check(self, who, ref=None, allowed=None):
        """ref, allowed: the float64 reference [Z][m][n] and the allowed error - needed with r_is_c, where the result arrives
        holding the residual: a word may keep its bits only where the residual itself is an allowed value of the result (a
        product, or a GELU of a far negative value, that vanishes beside it)"""
        may_keep = None
        if self.form == 0 and self.c["r_is_c"]:
            r = self.op.sent["out"][self.at]
            may_keep = np.zeros(self.own.size, bool)
            may_keep[self.at.reshape(-1)] = (np.abs(ref - r) <= allowed).reshape(-1)
        return self.op.check_words(who, {self.key: self.own}, may_keep)

    def session(self, z):
        """the bits of operand set z's result"""
        if self.key == "out":
            return bits(self.result[self.at[z]])
        return self.result[self.off3[z]:self.off3[z] + self.words]


def one_session(c, z):
    s = dict(c)
    s.update(batch=0, name=f"{c['name']}[{z}]")
    for key in ("a", "r", "x", "qkv"):
        if s.get(key) is not None:
            s[key] = c[key][z:z + 1]
    return s


REFS = {}


def refs(c):
    """the float64 reference and the float32 restatement of a case, computed once"""
    if c["name"] not in REFS:
        REFS.clear()
        REFS[c["name"]] = (EC.reference(c, np.float64), EC.reference(c, np.float32))
    return REFS[c["name"]]


def same_bits(a, b):
    return a.rc == 0 and b.rc == 0 and np.array_equal(bits(a.result), bits(b.result))


# ----------------------------------------------------------------------------------------------------------------------
# the X3 GEMM
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.GEMM_NAMES)
def test_gemm(name):
    c = EC.case(name)
    ref, f32 = refs(c)
    failures, rep = [], dict(form=c["form"], batch=c["batch"])
    walks = c["walks"]
    first = Gemm(c, walks[0])
    assert first.rc == 0, first.msg
    failures += first.check(f"walk {walks[0]}", ref, ER.allowed_error(ref, f32, EC.family(c))[0])
    got, canonical = first.values()
    entry, fail = ER.judge(name, got, ref, f32, EC.family(c))
    rep.update(entry, guards="ok" if not failures else "FAILED", canonical=canonical)
    print(name, json.dumps(rep))
    if fail:
        failures.append(fail)
    if not canonical:
        failures.append("the X3 result is not the canonical split of float32 values (or a pad key is not + 0)")
    identities = {}
    for walk in walks[1:]:          # tile height, persistent or one workgroup per tile, column- or row-major: the same bits
        other = Gemm(c, walk)
        identities[f"walk{walk}"] = same_bits(other, first)
    identities["repeated"] = same_bits(Gemm(c, walks[0]), first)
    if c["batch"] >= 1:             # session z of a table launch is that session alone with plain pointers
        for z in range(c["batch"]):
            one = Gemm(one_session(c, z), walks[0])
            identities[f"session{z}_alone"] = one.rc == 0 and np.array_equal(one.session(0), first.session(z))
    if c["form"]:                   # the decoded image is the fp32-result call with the same flags, bit for bit
        plain = Gemm(c, walks[0], form=0)
        identities["image_is_fp32_result"] = plain.rc == 0 and np.array_equal(got, plain.values()[0])
    rep["identities"] = identities
    failures += [f"bit identity broken: {k}" for k, ok in identities.items() if not ok]
    report(name, rep)
    assert not failures, "\n".join(failures)


def test_gemm_rows_do_not_depend_on_what_is_stacked_under_them():
    """rows 0 .. 63 of an M = 97 call are the M = 64 call (csrc/gemm_x3.hip: "Rows do not depend on what is stacked under them")"""
    for name in [n for n in EC.GEMM_NAMES if EC.SPECS[n]["m"] == 97 and EC.SPECS[n]["form"] == 0 and EC.SPECS[n]["k"] < 1024]:
        c = EC.case(name)
        top = dict(c, m=64, a=c["a"][:, :64], r=None if c["r"] is None else c["r"][:, :64])
        for walk in ((96, 1, 1), (64, 1, 1)):
            a, b = Gemm(c, walk), Gemm(top, walk)
            assert a.rc == 0 and b.rc == 0, (a.msg, b.msg)
            assert np.array_equal(bits(a.result[a.at[:, :64]]), bits(b.result[b.at])), (name, walk)


# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ----------------------------------------------------------------------------------------------------------------------
class LayerNorm:
    def __init__(self, c, form, **override):
        Z, rows, d = max(c["batch"], 1), c["rows"], c["d"]
        self.c, self.form, self.Z = c, form, Z
        ldx = d + 4
        x_off, x_size = offsets(rows * ldx, Z, 4)
        x = guard(x_size)
        for z in range(Z):
            x[x_off[z]:x_off[z] + rows * ldx].reshape(rows, ldx)[:, :d] = c["x"][z]
        kw = dict(kind=_lib.ENC_LN, form=form, m=rows, n=d, batch=c["batch"], ld_in=ldx, in_off=x_off, w=guarded(c["gamma"]),
                  bias=guarded(c["beta"]))
        kw["in"] = x
        if form == 0:
            ldy = d + 4
            off, size = offsets(rows * ldy, Z, 3)
            self.at = np.stack([off[z] + np.arange(rows)[:, None] * ldy + np.arange(d)[None, :] for z in range(Z)])
            self.own = np.zeros(size, bool)
            self.own[self.at.reshape(-1)] = True
            kw.update(out=guard(size), ld_out=ldy, out_off=off)
            self.key = "out"
        else:
            self.ld3 = d + 8
            self.words = rows * 3 * self.ld3
            self.off3, size = offsets(self.words, Z, 8)
            self.own = np.zeros(size, bool)
            for z in range(Z):
                self.own |= ER.owned_words("rows", size, rows=rows, cols=d, ld=self.ld3, at=self.off3[z])
            kw.update(out3=guard16(size), ld_out3=self.ld3, out3_off=self.off3)
            self.key = "out3"
        kw.update(override)
        self.op = Op(c["name"], **kw)
        self.rc, self.msg = self.op.rc, self.op.msg

    @property
    def result(self):
        return self.op.buf[self.key]

    def session(self, z):
        """the bits of operand set z's result"""
        if self.key == "out":
            return bits(self.result[self.at[z]])
        return self.result[self.off3[z]:self.off3[z] + self.words]

    def values(self):
        if self.form == 0:
            return self.result[self.at].astype(np.float64), True
        out, ok = np.empty((self.Z, self.c["rows"], self.c["d"])), True
        for z in range(self.Z):
            out[z], can = ER.decode_rows(self.result[self.off3[z]:], self.c["rows"], self.c["d"], self.ld3)
            ok = ok and bool(can.all())
        return out, ok


@pytest.mark.parametrize("name", EC.LN_NAMES)
def test_layernorm(name):
    c = EC.case(name)
    ref, f32 = refs(c)
    failures, rep, got = [], dict(batch=c["batch"]), {}
    for form in (0, 1):
        tag = ("fp32", "x3")[form]
        call = LayerNorm(c, form)
        assert call.rc == 0, call.msg
        failures += call.op.check_words(tag, {call.key: call.own})
        got[form], canonical = call.values()
        entry, fail = ER.judge(f"{name} {tag}", got[form], ref, f32, EC.family(c))
        rep[tag] = entry
        print(name, tag, json.dumps(entry))
        failures += [fail] if fail else []
        if not canonical:
            failures.append(f"{tag}: the image is not the canonical split of float32 values")
        identities = dict(repeated=same_bits(LayerNorm(c, form), call))
        if c["batch"] >= 1:
            for z in range(c["batch"]):
                one = LayerNorm(one_session(c, z), form)
                identities[f"session{z}_alone"] = one.rc == 0 and np.array_equal(one.session(0), call.session(z))
        rep[tag]["identities"] = identities
        failures += [f"{tag}: bit identity broken: {k}" for k, ok in identities.items() if not ok]
    # the decoded image is launch_layernorm's fp32 rows, bit for bit (decoded on the host, not by the device's unpack kernel)
    rep["x3_is_fp32"] = bool(np.array_equal(got[0], got[1]))
    if not rep["x3_is_fp32"]:
        failures.append(f"the X3 LayerNorm differs from the fp32 one in {int((got[0] != got[1]).sum())} values")
    rep["guards"] = "ok" if not any("wrote" in f or "unwritten" in f or "inputs" in f for f in failures) else "FAILED"
    report(name, rep)
    assert not failures, "\n".join(failures)


# ----------------------------------------------------------------------------------------------------------------------
# attention
# ----------------------------------------------------------------------------------------------------------------------
class Attention:
    def __init__(self, c, x3_out=False, in3=None, in3_off=None, **override):
        Z, T, d = max(c["batch"], 1), c["T"], c["d"]
        self.c, self.Z, self.x3_out = c, Z, x3_out
        kw = dict(kind=_lib.ENC_ATTENTION, form=c["form"], m=T, n=d, n_head=c["H"], batch=c["batch"], x3_out=int(x3_out))
        if in3 is not None:
            kw.update(in3=in3, in3_off=in3_off)
        else:
            q_off, q_size = offsets(T * 3 * d, Z, 4)
            qkv = guard(q_size)
            for z in range(Z):
                qkv[q_off[z]:q_off[z] + T * 3 * d] = c["qkv"][z].reshape(-1)
            kw["in"] = qkv
            kw["in_off"] = q_off
        if x3_out:
            self.ld3 = d + 8
            self.words = T * 3 * self.ld3
            self.off3, size = offsets(self.words, Z, 8)
            self.own = np.zeros(size, bool)
            for z in range(Z):
                self.own |= ER.owned_words("rows", size, rows=T, cols=d, ld=self.ld3, at=self.off3[z])
            kw.update(out3=guard16(size), ld_out3=self.ld3, out3_off=self.off3)
            self.key = "out3"
        else:
            ldo = d if c["form"] == 0 else d + 8         # (launch_encoder_attention writes rows d apart)
            off, size = offsets(T * ldo, Z, 4)
            self.at = np.stack([off[z] + np.arange(T)[:, None] * ldo + np.arange(d)[None, :] for z in range(Z)])
            self.own = np.zeros(size, bool)
            self.own[self.at.reshape(-1)] = True
            kw.update(out=guard(size), ld_out=ldo, out_off=off)
            self.key = "out"
        kw.update(override)
        self.op = Op(c["name"], **kw)
        self.rc, self.msg = self.op.rc, self.op.msg

    @property
    def result(self):
        return self.op.buf[self.key]

    def session(self, z):
        """the bits of operand set z's result"""
        if self.key == "out":
            return bits(self.result[self.at[z]])
        return self.result[self.off3[z]:self.off3[z] + self.words]

    def values(self):
        if not self.x3_out:
            return self.result[self.at].astype(np.float64), True
        out, ok = np.empty((self.Z, self.c["T"], self.c["d"])), True
        for z in range(self.Z):
            out[z], can = ER.decode_rows(self.result[self.off3[z]:], self.c["T"], self.c["d"], self.ld3)
            ok = ok and bool(can.all())
        return out, ok


@pytest.mark.parametrize("name", EC.ATT_NAMES)
def test_attention(name):
    c = EC.case(name)
    ref, f32 = refs(c)
    failures, rep, got = [], dict(batch=c["batch"], T=c["T"], H=c["H"], inputs=c["inputs"]), {}
    for x3_out in (False, True) if c["form"] == 1 else (False,):
        tag = "x3_out" if x3_out else "fp32_out"
        call = Attention(c, x3_out)
        assert call.rc == 0, call.msg
        failures += call.op.check_words(tag, {call.key: call.own})
        got[x3_out], canonical = call.values()
        entry, fail = ER.judge(f"{name} {tag}", got[x3_out], ref, f32, EC.family(c))
        rep[tag] = entry
        print(name, tag, json.dumps(entry))
        failures += [fail] if fail else []
        if not canonical:
            failures.append(f"{tag}: the image is not the canonical split of float32 values")
        identities = dict(repeated=same_bits(Attention(c, x3_out), call))
        if c["batch"] >= 1:
            for z in range(c["batch"]):
                one = Attention(one_session(c, z), x3_out)
                identities[f"session{z}_alone"] = one.rc == 0 and np.array_equal(one.session(0), call.session(z))
        rep[tag]["identities"] = identities
        failures += [f"{tag}: bit identity broken: {k}" for k, ok in identities.items() if not ok]
    if c["form"] == 1:
        rep["x3_out_is_fp32_out"] = bool(np.array_equal(got[False], got[True]))
        if not rep["x3_out_is_fp32_out"]:
            failures.append(f"the x3_out rows differ from the fp32 rows in {int((got[False] != got[True]).sum())} values")
    rep["guards"] = "ok" if not any("wrote" in f or "unwritten" in f or "inputs" in f for f in failures) else "FAILED"
    report(name, rep)
    assert not failures, "\n".join(failures)


QKV_FEEDS = tuple(n for n in EC.GEMM_NAMES if EC.SPECS[n]["form"] == 2 and EC.SPECS[n]["m"] >= 64)


@pytest.mark.parametrize("name", QKV_FEEDS)
def test_qkv_image_feeds_the_x3_attention(name):
    """the image the qkv form wrote - into a buffer that was never zeroed - is the X3 attention's operand in a second call"""
    c = EC.case(name)
    H = c["d"] // ER.HEAD
    proj = Gemm(c, c["walks"][0])
    assert proj.rc == 0, proj.msg
    qkv64, qkv32 = refs(c)
    att = dict(kind="attention", form=1, T=c["m"], H=H, d=c["d"], batch=c["batch"], name=name + "+attention", inputs="projection",
               qkv=proj.values()[0].astype(np.float32))
    fed = Attention(att, in3=proj.result.copy(), in3_off=proj.off3)
    assert fed.rc == 0, fed.msg
    assert not fed.op.changed(["in3"])
    ref, f32 = ER.attention(qkv64, H, np.float64), ER.attention(qkv32, H, np.float32)
    entry, fail = ER.judge(name, fed.values()[0], ref, f32, "attention_x3")
    packed = Attention(att)             # the same values packed by launch_x3_pack_qkv: the same image, the same bits
    entry["image_is_pack_qkv"] = same_bits(packed, fed)
    report(name + "+attention", entry)
    assert not fail and entry["image_is_pack_qkv"], (fail, entry)


# ----------------------------------------------------------------------------------------------------------------------
# pack
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.PACK_NAMES)
def test_pack(name):
    c = EC.case(name)
    rows, cols = c["rows"], c["cols"]
    ld_src, ld_dst = cols + 4, cols + 8
    src = guard(rows * ld_src + TAIL)
    src[:rows * ld_src].reshape(rows, ld_src)[:, :cols] = c["x"]
    size = rows * 3 * ld_dst + TAIL
    kw = dict(kind=_lib.ENC_PACK, m=rows, n=cols, ld_in=ld_src, ld_out3=ld_dst, out3=guard16(size))
    kw["in"] = src
    op = Op(name, **kw)
    assert op.rc == 0, op.msg
    own = ER.owned_words("rows", size, rows=rows, cols=cols, ld=ld_dst)
    failures = op.check_words("pack", {"out3": own})
    idx = ER._row_words(rows, cols, ld_dst)
    device = np.stack([op.buf["out3"][idx + 8 * p] for p in range(3)])
    host = ER.split(c["x"])
    inside = ER.split_exact(c["x"])
    differs = np.any(device != host, axis=0)
    outside = [dict(x=hex(int(b)), device=[hex(int(w)) for w in device[:, i, j]], host=[hex(int(w)) for w in host[:, i, j]])
               for (i, j), b in zip(np.argwhere(differs & ~inside), bits(c["x"])[differs & ~inside])]
    report(name, dict(values=int(inside.size), inside_domain=int(inside.sum()), differ_inside=int((differs & inside).sum()),
                      differ_outside=int((differs & ~inside).sum()), outside_examples=outside[:16],
                      guards="ok" if not failures else "FAILED"))
    if (differs & inside).any():
        i, j = np.argwhere(differs & inside)[0]
        failures.append(f"the device split of {hex(int(bits(c['x'])[i, j]))} is {[hex(int(w)) for w in device[:, i, j]]}, "
                        f"x3_split gives {[hex(int(w)) for w in host[:, i, j]]} ({int((differs & inside).sum())} values differ)")
    assert not failures, "\n".join(failures)


# ----------------------------------------------------------------------------------------------------------------------
# the production composition on small shapes
# ----------------------------------------------------------------------------------------------------------------------
def test_layer_composition():
    """X3 LayerNorm image -> qkv form -> X3 attention with x3_out -> out projection onto the residual stream (r_is_c):
    d = 128, H = 2, T = 97, three sessions, four calls that feed each other's returned buffers; against the float64 chain
    and against the same chain through the fp32 kernels"""
    d, H, T, Z = 128, 2, 97, 3
    rng = np.random.default_rng(24)
    x = (rng.standard_normal((Z, T, d)) + 0.3).astype(np.float32)
    gamma, beta = (1.0 + 0.2 * rng.standard_normal(d)).astype(np.float32), (0.1 * rng.standard_normal(d)).astype(np.float32)
    wqkv, bqkv = (rng.standard_normal((3 * d, d)) / np.sqrt(d)).astype(np.float32), (0.1 * rng.standard_normal(3 * d)).astype(np.float32)
    wout, bout = (rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32), (0.1 * rng.standard_normal(d)).astype(np.float32)
    scale = 0.3535533905932738

    def chain(dt):
        h = ER.layernorm(x, gamma, beta, dt)
        qkv = ER.gemm(h, wqkv, bqkv, ER.SCALE, scale, 2 * d, 0, None, dt)
        a = ER.attention(qkv, H, dt)
        return ER.gemm(a, wout, bout, ER.RESIDUAL, 1.0, 0, 0, x, dt)
    ref, f32 = chain(np.float64), chain(np.float32)

    ln_case = dict(name="layer.ln", kind="ln", batch=Z, rows=T, d=d, x=x, gamma=gamma, beta=beta)
    qkv_case = dict(name="layer.qkv", kind="gemm", form=2, batch=Z, m=T, n=3 * d, k=d, d=d, flags=ER.SCALE, scale=scale, scale_cols=2 * d,
                    scale_period=0, r_is_c=False, a=np.zeros((Z, T, d), np.float32), w=wqkv, bias=bqkv, r=None)
    att_case = dict(name="layer.attention", kind="attention", form=1, batch=Z, T=T, H=H, d=d, qkv=np.zeros((Z, T, 3 * d), np.float32))
    out_case = dict(name="layer.out", kind="gemm", form=0, batch=Z, m=T, n=d, k=d, d=d, flags=ER.RESIDUAL, scale=1.0, scale_cols=0,
                    scale_period=0, r_is_c=True, a=np.zeros((Z, T, d), np.float32), w=wout, bias=bout, r=x)
    ln = LayerNorm(ln_case, 1)
    assert ln.rc == 0, ln.msg
    kw_in = {"in": None}
    qkv = Gemm(qkv_case, in3=ln.result.copy(), in3_off=ln.off3, ld_in=ln.ld3, **kw_in)
    assert qkv.rc == 0, qkv.msg
    att = Attention(att_case, x3_out=True, in3=qkv.result.copy(), in3_off=qkv.off3, **kw_in)
    assert att.rc == 0, att.msg
    out = Gemm(out_case, in3=att.result.copy(), in3_off=att.off3, ld_in=att.ld3, **kw_in)
    assert out.rc == 0, out.msg
    failures = qkv.check("qkv") + out.check("out", ref, ER.allowed_error(ref, f32, "layer")[0]) + att.op.check_words("attention", {"out3": att.own})
    got = out.values()[0]
    entry, fail = ER.judge("layer x3", got, ref, f32, "layer")
    # the same layer through the fp32 kernels: LayerNorm rows -> fp32-result projection -> fp32 attention -> out projection
    ln32 = LayerNorm(ln_case, 0)
    q32 = Gemm(dict(qkv_case, a=ln32.values()[0].astype(np.float32)), form=0)
    a32 = Attention(dict(att_case, form=0, qkv=q32.values()[0].astype(np.float32)))
    o32 = Gemm(dict(out_case, a=a32.values()[0].astype(np.float32)))
    assert ln32.rc == 0 and q32.rc == 0 and a32.rc == 0 and o32.rc == 0, (ln32.msg, q32.msg, a32.msg, o32.msg)
    entry32, fail32 = ER.judge("layer fp32", o32.values()[0], ref, f32, "layer")
    allowed, _ = ER.allowed_error(ref, f32, "layer")
    between = ER.abs_err(got, o32.values()[0])
    rep = dict(x3=entry, fp32=entry32, x3_vs_fp32=float(between.max()), guards="ok" if not failures else "FAILED")
    print("layer", json.dumps(rep))
    report("layer_composition", rep)
    failures += [f for f in (fail, fail32) if f]
    if (between > 2 * allowed).any():
        failures.append(f"the two chains differ by {between.max():.3e}, more than both tolerances together")
    assert not failures, "\n".join(failures)


# ----------------------------------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", list(EC.REFUSALS))
def test_refusals(what):
    base, override, fragment = EC.REFUSALS[what]
    c = EC.case(base)
    call = Attention(c, **override) if c["kind"] == "attention" else Gemm(c, **override)
    assert call.rc == WLK_ERR_ARG and fragment in call.msg, (what, call.rc, call.msg)
    assert not call.op.changed(), "a refused call touched a buffer"
