"""NLLB's ragged decoder cross-attention (csrc/nllb_batch.hip: nllb_cross_attention_ragged_kernel<false|true>) through
wlk_diag_nllb_cross_ragged - the two production launchers, unchanged - against the float64 statement of
tests/cross_ragged_reference.py on the cases of tests/cross_ragged_cases.py: every key count around the 16-key pass of
the four waves, the 128-key preload (beyond it keys are loaded inside the loop) and the bound of 512, alone and eight to a
launch.  No model, no batch object.

Tolerance (tests/select_reference.py: value_tolerance): 4 x the float32 restatement's error on the case, floor 2^-22 *
max(1, |reference|), for the outputs, the stored weights and their sums.  Bit identities: the align form's output is the
plain form's; a row's output and weights are those of the same row alone.  Every buffer carries guard words - a NaN bit
pattern - behind it and between the K/V blocks, key rows at and beyond a row's length and the other layers' columns are
NaN, the alignment block arrives filled with the pattern and keeps it wherever no weight belongs.  Every case writes its
figures to cross_ragged_report.json in the directory WLK_REPORT_DIR names (default: test_reports/)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import cross_ragged_cases as RC
import cross_ragged_reference as RR
from whisperlivekit_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}
WLK_ERR_ARG = -1
GUARD = np.uint32(0x7FC12345)
TAIL = 3
GAP = 8                                 # guard words between two K/V blocks (a multiple of 4: blocks stay 16-byte aligned)
POINTERS = ("q", "kv", "out", "align_probs", "head_rank")


def report(key, value):
    REPORT[key] = value
    out = os.environ.get("WLK_REPORT_DIR") or os.path.join(ROOT, "test_reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "cross_ragged_report.json"), "w") as fh:
        json.dump(REPORT, fh, indent=1, sort_keys=True)


def guard(n):
    return np.full(n, GUARD, np.uint32).view(np.float32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


class Run:
    """one wlk_diag_nllb_cross_ragged call on a case; keeps what was sent"""

    def __init__(self, c, align, **override):
        R, d, H = c["n_rows"], c["d"], c["H"]
        self.c, self.align = c, align
        kv_at, at = [], 0
        for b in c["blocks"]:
            kv_at.append(at)
            at += b.size + GAP
        kv = guard(at + TAIL)
        for b, o in zip(c["blocks"], kv_at):
            kv[o:o + b.size] = b.reshape(-1)
        q = guard(R * d + TAIL)
        q[:R * d] = c["q"].reshape(-1)
        self.np_ = c["n_rank"] * RR.MAX_ROWS * c["stride"]
        self.buf = dict(q=q, kv=kv, out=guard(R * d + TAIL), align_probs=guard(self.np_ + TAIL) if align else None,
                        head_rank=c["head_rank"].copy() if align else None)
        self.lengths = np.ascontiguousarray(c["lengths"], np.int32)
        self.kv_at = np.asarray(kv_at, np.int64)
        self.kv_rows = np.asarray(c["kv_rows"], np.int32)
        kw = dict(n_rows=R, d=d, n_head=H, align=int(align), n_rank=c["n_rank"], align_stride=c["stride"], kv_off=c["kv_off"],
                  ldkv=c["ldkv"], q_floats=q.size, kv_floats=kv.size, out_floats=self.buf["out"].size,
                  probs_floats=self.np_ + TAIL if align else 0)
        for key in list(override):
            if key in ("lengths", "kv_at", "kv_rows"):
                setattr(self, key, override.pop(key))
            elif key in POINTERS:
                self.buf[key] = override.pop(key)
        kw.update(override)
        self.sent = {key: None if v is None else v.copy() for key, v in self.buf.items()}
        args = _lib.DiagNllbCrossRaggedArgs()
        for key, v in self.buf.items():
            if v is not None:
                setattr(args, key, v.ctypes.data)
        args.lengths, args.kv_at, args.kv_rows = self.lengths.ctypes.data, self.kv_at.ctypes.data, self.kv_rows.ctypes.data
        for key, val in kw.items():
            setattr(args, key, val)
        lib = _lib.load()
        self.rc = lib.wlk_diag_nllb_cross_ragged(C.byref(args))
        self.msg = "" if self.rc == 0 else lib.wlk_diag_last_error().decode()
        if self.rc not in (0, WLK_ERR_ARG):     # a HIP error: the device's state is unknown, nothing more is launched on it
            pytest.exit(f"wlk_diag_nllb_cross_ragged ({c['name']}): error {self.rc}: {self.msg}", returncode=3)

    def changed(self, keys=POINTERS):
        return [k for k in keys if self.sent[k] is not None and not np.array_equal(bits(self.buf[k]), bits(self.sent[k]))]

    def out(self):
        R, d = self.c["n_rows"], self.c["d"]
        return self.buf["out"][:R * d].reshape(R, d).copy()

    def raw(self):
        c = self.c
        return bits(self.buf["align_probs"][:self.np_]).reshape(c["n_rank"], RR.MAX_ROWS, c["stride"])

    def probs(self):
        """-> (weights [n_rank][8][stride], NaN where the guard still stands; words written that no weight belongs to)"""
        c = self.c
        p = self.buf["align_probs"][:self.np_].reshape(c["n_rank"], RR.MAX_ROWS, c["stride"])
        kept = bits(p) == GUARD
        return np.where(kept, np.nan, p.astype(np.float64)), kept

    def words(self, ref):
        fails = [f"changed its input {k}" for k in self.changed(("q", "kv", "head_rank"))]
        n = self.c["n_rows"] * self.c["d"]
        now = bits(self.buf["out"])
        if (now[n:] != GUARD).any():
            fails.append("wrote behind out")
        if (now[:n] == GUARD).any():
            fails.append(f"left {int((now[:n] == GUARD).sum())} words of out unwritten")
        if self.align:
            if (bits(self.buf["align_probs"])[self.np_:] != GUARD).any():
                fails.append("wrote behind align_probs")
            _, kept = self.probs()
            owned = ~np.isnan(ref["probs"])
            if (kept != ~owned).any():
                fails.append(f"{int((~kept & ~owned).sum())} alignment words written that no weight belongs to (rows at or beyond "
                             f"n_rows, columns at or beyond a row's length, ranks no head has), {int((kept & owned).sum())} weights missing")
        return fails


@pytest.mark.parametrize("name", RC.NAMES)
def test_outputs_and_weights_against_float64(name):
    c = RC.case(name)
    ref, f32 = RR.attention(c), RR.attention(c, np.float32)
    plain, align = Run(c, False), Run(c, True)
    assert plain.rc == 0 and align.rc == 0, (plain.msg, align.msg)
    fails = [f"plain: {f}" for f in plain.words(ref)] + [f"align: {f}" for f in align.words(ref)]
    probs, _ = align.probs()
    sums = ref["sums"].copy()           # of the kept heads, the stored weights' sum; the others keep the reference's 1
    for h, rank in enumerate(c["head_rank"]):
        if rank >= 0:
            sums[:, h] = np.nansum(probs[rank, :c["n_rows"]].astype(np.float64), axis=1)
    rep, f = RR.compare(ref, f32, dict(out=plain.out(), probs=probs, sums=sums))
    fails += f
    print(name, json.dumps(rep))
    report(name, rep)
    if not np.array_equal(bits(plain.out()), bits(align.out())):
        fails.append("the align form's output is not the plain form's, bit for bit")
    if c["style"] == "peak":            # the output is the value row of the key 60 above the rest
        want = np.empty_like(ref["out"])
        for r in range(c["n_rows"]):
            for h in range(c["H"]):
                sl = slice(h * 64, (h + 1) * 64)
                want[r, sl] = c["blocks"][r][c["peak"][r, h], c["kv_off"] + c["d"]:c["kv_off"] + 2 * c["d"]][sl]
        fails += [f"against the peak key's value row: {x}" for x in RR.compare(dict(out=want), dict(out=f32["out"]), dict(out=plain.out()))[1]]
    if c["n_rows"] > 1:                 # a row alone: the same bits, also beyond the 128 preloaded keys
        for r in range(c["n_rows"]):
            one = Run(RC.alone(c, r), True)
            assert one.rc == 0, one.msg
            if not np.array_equal(bits(one.out()[0]), bits(align.out()[r])):
                fails.append(f"row {r} ({int(c['lengths'][r])} keys) alone gives other output bits")
            if not np.array_equal(one.raw()[:, 0], align.raw()[:, r]):
                fails.append(f"row {r} ({int(c['lengths'][r])} keys) alone stores other weights")
    else:
        again = Run(c, True)
        if not (np.array_equal(bits(again.buf["out"]), bits(align.buf["out"])) and np.array_equal(again.raw(), align.raw())):
            fails.append("a second launch gives other bits")
    assert not fails, "\n".join(fails)


def test_refusals_come_before_anything_is_uploaded():
    c = RC.case("mixed_g0")
    nine = dict(c)
    nine.update(n_rows=9, lengths=np.append(c["lengths"], 3).astype(np.int32), kv_rows=c["kv_rows"] + [c["kv_rows"][2]],
                blocks=c["blocks"] + [c["blocks"][2]], q=np.concatenate([c["q"], c["q"][:1]]))
    lengths = lambda i, v: np.where(np.arange(c["n_rows"]) == i, v, c["lengths"]).astype(np.int32)
    ranks = lambda v: np.where(np.arange(c["H"]) == 0, v, c["head_rank"]).astype(np.int32)
    for case, align, override, text in [
            (c, False, dict(lengths=lengths(3, 0)), "a row has 1 .. 512 keys"),
            (c, False, dict(lengths=lengths(7, 513)), "a row has 1 .. 512 keys"),
            (c, True, dict(lengths=lengths(0, -1)), "a row has 1 .. 512 keys"),
            (nine, True, {}, "the alignment rows hold 8 rows"),
            (c, True, dict(align_stride=513), "the alignment rows hold 8 rows"),
            (c, True, dict(align_stride=16), "more keys than an alignment row holds"),
            (c, False, dict(d=c["d"] + 64), "d = 64 n_head"),
            (c, False, dict(n_head=c["H"] + 1), "d = 64 n_head"),
            (c, False, dict(ldkv=c["kv_off"] + 2 * c["d"] - 4), "a key row does not hold k | v at kv_off"),
            (c, False, dict(kv_off=c["ldkv"] - 2 * c["d"] + 4), "a key row does not hold k | v at kv_off"),
            (c, False, dict(kv_off=2), "a key row does not hold k | v at kv_off"),
            (c, True, dict(head_rank=ranks(c["n_rank"])), "a head's rank lies outside"),
            (c, True, dict(head_rank=ranks(-2)), "a head's rank lies outside"),
            (c, False, dict(kv_rows=np.asarray(c["kv_rows"], np.int32) - 3), "holds fewer rows than the row's length"),
            (c, False, dict(kv_floats=100), "a K/V block lies past kv"),
            (c, False, dict(out_floats=c["n_rows"] * c["d"] - 1), "q / out hold fewer"),
            (c, True, dict(probs_floats=c["n_rank"] * 8 * c["stride"] - 1), "align_probs holds fewer"),
            (c, True, dict(align_probs=None), "the align form needs head_rank")]:
        run = Run(case, align, **override)
        assert run.rc == WLK_ERR_ARG and text in run.msg, (override, run.rc, run.msg)
        assert not run.changed(), (override, "a refused call changed a buffer")
    assert Run(nine, False).rc == 0         # the plain form takes more than 8 rows (a stacked prefill)
