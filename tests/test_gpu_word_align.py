"""The device half of find_alignment behind the vocabulary projection (csrc/word_align.hip: token probabilities, softmax
over the content frames, z-score over the token rows, median of 7 + head mean, the hand-over to dtw) through
wlk_diag_word_align - the production launcher launch_word_align, unchanged, stopped after each stage in turn - against the
float64 statement of tests/word_align_reference.py on the cases of tests/word_align_cases.py.  No model, no session.

Tolerance (tests/select_reference.py: value_tolerance): a value may be off by 4 x the error the float32 restatement has on
the same case (floor 2^-22 * max(1, |reference|)); a NaN must stand exactly where the reference has one.  Bit identities:
the z of a later stage is the z of the z-score stage; cost is the float32 recomputation from the kernel's own z (median by
selection, heads added in ascending order, one division, the negation); the trace is timing_oracle.dtw_trace of the
kernel's own cost in every cell, border included; a second launch repeats the first.  Every buffer carries guard words - a
NaN bit pattern - behind it and arrives filled with them where it is a result; the scores hold NaN at and beyond F and P, the
logits 1e30 at and beyond n_cols.  Every case writes its figures to word_align_report.json in the directory WLK_REPORT_DIR
names (default: test_reports/)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import word_align_cases as WC
import word_align_reference as WR
from oracle import timing_oracle
from whisperlivekit_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}
WLK_ERR_ARG = -1
GUARD = np.uint32(0x7FC12345)           # a NaN with a payload: reading it poisons, and it is recognisable
TGUARD, BGUARD = np.int32(-77777), np.int8(0x55)
TAIL = 3
STAGES = (_lib.WA_SOFTMAX, _lib.WA_ZSCORE, _lib.WA_COST, _lib.WA_DTW)
POINTERS = ("ring", "logits", "targets", "w", "cost", "probs", "trace")
SIZES = dict(zip(POINTERS, ("ring_floats", "logits_floats", "targets_n", "w_floats", "cost_floats", "probs_floats", "trace_bytes")))


def report(key, value):
    REPORT[key] = value
    out = os.environ.get("WLK_REPORT_DIR") or os.path.join(ROOT, "test_reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "word_align_report.json"), "w") as fh:
        json.dump(REPORT, fh, indent=1, sort_keys=True)


def guard(n):
    return np.full(n, GUARD, np.uint32).view(np.float32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def guarded(a):
    a = np.ascontiguousarray(a, np.float32)
    buf = guard(a.size + TAIL)
    buf[:a.size] = a.reshape(-1)
    return buf


class Run:
    """one wlk_diag_word_align call on a case; keeps what was sent"""

    def __init__(self, c, stage, **override):
        A, P, F, n_text = c["n_align"], c["P"], c["F"], c["n_text"]
        self.c, self.stage = c, stage
        self.nw, self.nc, self.nt = A * P * F, (n_text + 1) * F, (n_text + 2) * (F + 1)
        targets = np.full(n_text + TAIL, TGUARD, np.int32)
        targets[:n_text] = c["targets"]
        self.buf = dict(ring=guarded(c["ring"]), logits=guarded(c["logits"]), targets=targets, w=guard(self.nw + TAIL),
                        cost=guard(self.nc + TAIL), probs=guard(n_text + TAIL), trace=np.full(self.nt + TAIL, BGUARD, np.int8))
        kw = dict(P=P, F=F, T=c["T"], ring_rows=c["ring_rows"], n_align=A, n_sot=c["n_sot"], n_cols=c["n_cols"], last_stage=stage,
                  qk_scale=c["qk_scale"], ld=c["ld"])
        sizes = {}
        for key in list(override):
            if key in POINTERS:
                self.buf[key] = override.pop(key)
            elif key in SIZES.values():
                sizes[key] = override.pop(key)
        kw.update(override)
        self.sent = {key: None if v is None else v.copy() for key, v in self.buf.items()}
        args = _lib.DiagWordAlignArgs()
        for key, v in self.buf.items():
            if v is not None:
                setattr(args, key, v.ctypes.data)
                setattr(args, SIZES[key], v.size)
        for key, val in {**kw, **sizes}.items():
            setattr(args, key, val)
        lib = _lib.load()
        self.rc = lib.wlk_diag_word_align(C.byref(args))
        self.msg = "" if self.rc == 0 else lib.wlk_diag_last_error().decode()
        if self.rc not in (0, WLK_ERR_ARG):     # a HIP error: the device's state is unknown, nothing more is launched on it
            pytest.exit(f"wlk_diag_word_align ({c['name']}): error {self.rc}: {self.msg}", returncode=3)

    def unchanged(self, keys=POINTERS):
        return [k for k in keys if self.sent[k] is not None and not np.array_equal(bits(self.buf[k]), bits(self.sent[k]))]

    def words(self):
        """-> failures: an input changed, a guard word behind a result written, a result the stage does not reach written,
        an owned word that still holds the guard"""
        fails = [f"changed its input {k}" for k in self.unchanged(("ring", "logits", "targets"))]
        owned = dict(w=self.nw, probs=self.c["n_text"], cost=self.nc if self.stage >= _lib.WA_COST else 0,
                     trace=self.nt if self.stage >= _lib.WA_DTW else 0)
        for key, n in owned.items():
            now, sent = bits(self.buf[key]), bits(self.sent[key])
            if not np.array_equal(now[n:], sent[n:]):
                fails.append(f"wrote {int((now[n:] != sent[n:]).sum())} words of {key} it does not own")
            if (now[:n] == sent[:n]).any():
                fails.append(f"left {int((now[:n] == sent[:n]).sum())} owned words of {key} unwritten")
        return fails

    def got(self):
        c = self.c
        out = dict(probs=self.buf["probs"][:c["n_text"]].copy())
        body = self.buf["w"][:self.nw].reshape(c["n_align"], c["P"], c["F"]).copy()
        out["w" if self.stage == _lib.WA_SOFTMAX else "z"] = body
        if self.stage >= _lib.WA_COST:
            out["cost"] = self.buf["cost"][:self.nc].reshape(c["n_text"] + 1, c["F"]).copy()
        if self.stage >= _lib.WA_DTW:
            out["trace"] = self.buf["trace"][:self.nt].reshape(c["n_text"] + 2, c["F"] + 1).copy()
        return out


@pytest.mark.parametrize("name", WC.NAMES)
def test_every_stage_against_float64(name):
    c = WC.case(name)
    ref, f32 = WR.chain(c), WR.chain(c, np.float32)
    fails, rep, got = [], {}, {}
    for stage in STAGES:
        run = Run(c, stage)
        assert run.rc == 0, run.msg
        fails += [f"stage {stage}: {f}" for f in run.words()]
        got[stage] = run.got()
        r, f = WR.compare(ref, f32, got[stage])
        rep.update({f"{key}@{stage}": val for key, val in r.items()})
        fails += [f"stage {stage}: {x}" for x in f]
    print(name, json.dumps(rep))
    report(name, rep)
    z = got[_lib.WA_ZSCORE]["z"]
    last = got[_lib.WA_DTW]
    for stage in (_lib.WA_COST, _lib.WA_DTW):
        if not np.array_equal(bits(got[stage]["z"]), bits(z)):
            fails.append(f"the z of stage {stage} is not the z of the z-score stage")
        if not np.array_equal(bits(got[stage]["probs"]), bits(got[_lib.WA_SOFTMAX]["probs"])):
            fails.append(f"the probabilities of stage {stage} are not those of the softmax stage")
    if not np.array_equal(bits(last["cost"]), bits(got[_lib.WA_COST]["cost"])):
        fails.append("the cost of the dtw stage is not the cost of the cost stage")
    # NaN: exactly where the float64 statement has one - the planted columns of z, nothing from the plants beyond F / P
    planted = np.zeros((c["n_align"], c["F"]), bool)
    for a, f in c["nan_cols"]:
        planted[a, f] = True
    if c["F"] > 1 and not np.array_equal(np.isnan(z), np.broadcast_to(planted[:, None, :], z.shape)):
        fails.append("z is not NaN exactly in the planted columns")
    # cost from the kernel's own z, in float32: bit for bit where z is finite, NaN for NaN otherwise
    again = WR.cost_from_z(z, c["n_sot"], np.float32)
    if np.isnan(z).any():
        if not np.array_equal(again, last["cost"], equal_nan=True):
            fails.append("cost is not the float32 recomputation from z with a NaN ordered last")
    elif not np.array_equal(bits(again), bits(last["cost"])):
        fails.append(f"cost differs from the float32 recomputation from z in {int((bits(again) != bits(last['cost'])).sum())} words")
    want = timing_oracle.dtw_trace(last["cost"])
    if not np.array_equal(last["trace"], want):
        fails.append(f"the trace differs from dtw_trace of the kernel's cost in {int((last['trace'] != want).sum())} cells")
    if not ((last["trace"][0] == -1).all() and (last["trace"][:, 0] == -1).all()):
        fails.append("the trace's border is not -1")
    if name not in WC.BIG:
        rerun = Run(c, _lib.WA_DTW).got()
        for key in ("probs", "z", "cost", "trace"):
            if not np.array_equal(bits(rerun[key]), bits(last[key])):
                fails.append(f"a second launch gives another {key}")
    assert not fails, "\n".join(fails)


def test_refusals_of_the_check_function_and_of_the_buffers():
    c = WC.case("chain_p6_f5_a1")           # P = 6, n_sot = 3: one text token
    n_text = c["n_text"]
    bad_target = np.full(n_text + TAIL, TGUARD, np.int32)
    cases = [
        (dict(n_sot=0, P=3), "word alignment: need [sot sequence"),
        (dict(n_sot=4), "word alignment: need [sot sequence"),
        (dict(ring_rows=c["P"] - 1), "more token rows than the score window holds"),
        (dict(F=c["T"] + 1), "frames outside [1, T]"),
        (dict(n_align=0), "n_align in [1, 64]"),
        (dict(ld=c["n_cols"] - 1), "logit rows shorter than their columns"),
        (dict(last_stage=4), "last stage in [0, 3]"),
        (dict(last_stage=-1), "last stage in [0, 3]"),
        (dict(cost=None), "null cost matrix"),
        (dict(trace=None), "null trace"),
        (dict(targets=np.where(np.arange(n_text + TAIL) < n_text, c["n_cols"], bad_target).astype(np.int32)), "target outside the logit columns"),
        (dict(targets=np.where(np.arange(n_text + TAIL) < n_text, -1, bad_target).astype(np.int32)), "target outside the logit columns"),
        (dict(w_floats=c["n_align"] * c["P"] * c["F"] - 1), "w holds fewer"),
        (dict(cost_floats=(n_text + 1) * c["F"] - 1), "cost holds fewer"),
        (dict(trace_bytes=(n_text + 2) * (c["F"] + 1) - 1), "trace holds fewer"),
        (dict(probs_floats=n_text - 1), "probs holds fewer"),
        (dict(ring_floats=c["n_align"] * c["ring_rows"] * c["T"] - 1), "ring holds fewer"),
        (dict(logits_floats=(n_text - 1) * c["ld"] + c["n_cols"] - 1), "the logit rows lie past"),
        (dict(targets_n=n_text - 1), "targets holds fewer"),
    ]
    for override, text in cases:
        run = Run(c, override.pop("last_stage", _lib.WA_DTW), **override)
        assert run.rc == WLK_ERR_ARG and text in run.msg, (override, run.rc, run.msg)
        assert not run.unchanged(), (override, "a refused call changed a buffer")
    ok = Run(c, _lib.WA_ZSCORE, cost=None, trace=None)       # what a stage does not write may be absent
    assert ok.rc == 0, ok.msg


def test_refusals_of_find_alignment():
    import helpers
    from whisperlivekit_amd.dims import ALIGNMENT_HEADS, MODEL_DIMS
    from whisperlivekit_amd.engine import HipWhisperModel
    dims = MODEL_DIMS["micro.en"]
    model = HipWhisperModel.from_state_dict(dims, helpers.synth_sd("micro.en", 0), ALIGNMENT_HEADS["micro.en"], device=0)
    sess, beam2 = model.new_session(beam=1, batched=False), model.new_session(beam=2, batched=False)
    lib = _lib.load()
    eot, sot, nots = 50256, 50257, 50362

    def call(s, tokens, n_sot, eot_, num_frames):
        toks = np.asarray(tokens, np.int64)
        n_text = max(len(toks) - n_sot - 2, 1)
        f = max(num_frames // 2, 1)
        trace, probs = np.empty((n_text + 2) * (f + 1), np.int8), np.empty(n_text, np.float32)
        rc = lib.wlk_find_alignment(s._h, toks.ctypes.data_as(C.POINTER(C.c_int64)), len(toks), n_sot, eot_, num_frames, 1.0, None,
                                    trace.ctypes.data_as(C.POINTER(C.c_int8)), probs.ctypes.data_as(C.POINTER(C.c_float)))
        return rc, (lib.wlk_last_error() or b"").decode()

    good = [sot, nots, 100, 200, eot]
    try:
        rc, msg = call(sess, good, 1, eot, 400)
        assert rc != 0 and "before an encode" in msg, (rc, msg)
        for s in (sess, beam2):
            s.encode_mel(np.random.default_rng(0).standard_normal((dims.n_mels, 3000)).astype(np.float32))
        for s, tokens, n_sot, eot_, frames, text in [
                (sess, good, 0, eot, 400, "need [sot sequence"),
                (sess, [sot, nots, eot], 1, eot, 400, "need [sot sequence"),
                (sess, good, 1, eot, 1, "num_frames out of range"),
                (sess, good, 1, eot, 2 * dims.n_audio_ctx + 2, "num_frames out of range"),
                (sess, good, 1, 0, 400, "eot out of range"),
                (sess, good, 1, dims.n_vocab + 1, 400, "eot out of range"),
                (sess, [sot, nots, 100, eot, eot], 1, eot, 400, "text token >= eot"),
                (sess, [sot, nots, -1, 200, eot], 1, eot, 400, "text token >= eot"),
                (beam2, good, 1, eot, 400, "beam-1 session")]:
            rc, msg = call(s, tokens, n_sot, eot_, frames)
            assert rc == WLK_ERR_ARG and text in msg, (tokens, n_sot, eot_, frames, rc, msg)
        rc, msg = call(sess, good, 1, eot, 400)                 # and the session still aligns afterwards
        assert rc == 0, msg
    finally:
        sess.close()
        beam2.close()
        model.close()
