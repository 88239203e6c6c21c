"""The alignment-head survey on the GPU.

Kernel alone: csrc/head_survey.hip through wlk_diag_head_survey - the production launcher launch_head_survey, unchanged, no
model, no session - on the cases of tests/head_survey_cases.py against the float64 statement of
tests/head_survey_reference.py, with every key split (0 = the launcher's choice, 1, 2, the maximum).
  Values: denom = 1 / peak (>= 1) within select_reference.value_tolerance(ref = denom64, f32 = denom32): 4 x the error the
  float32 restatement has on the case, floor 2^-22 |ref|.
  Frames: the float64 arg-max exactly in every row (the generator keeps the top score >= 1e-3 ahead of the runner-up,
  test_head_survey_cpu.py asserts it); rows with bit-identical top keys demand the lowest index; all-equal rows frame 0.
  Buffers: a NaN-payload guard word behind every buffer, results arrive filled with guards, inputs come back bit for bit,
  nothing beyond [L][H][P] is written, every owned word is written, keys in [F, Tk) and every V half hold NaN; a second
  launch repeats the first bit for bit; every split gives the frames of split 1 and denominators within the tolerance.
Through the model (micro, synthetic weights): HipSession.head_survey against the session's debug export of the scores and
against oracle.whisper_oracle in float64; the session's state afterwards; every refusal; planted heads end to end through
collect_heads, the dump string and HipSimulStreamingASR; the command line.
A HIP error ends the test session (pytest.exit): the device's state is unknown, nothing more is launched.  Figures go to
head_survey_report.json in the directory WLK_REPORT_DIR names (default: test_reports/)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import head_survey_cases as HC
import select_reference as SR
from whisperlivekit_amd import _lib
from whisperlivekit_amd import alignment_heads as AH

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}
WLK_ERR_ARG, WLK_ERR_STATE, WLK_ERR_CAPACITY = -1, -3, -4
GUARD = np.uint32(0x7FC12345)           # a NaN with a payload: reading it poisons, and it is recognisable
IGUARD = np.int32(-77777)
TAIL = 3
POINTERS = ("q", "k", "peak", "frame")
SIZES = dict(q="q_floats", k="k_floats", peak="peak_floats", frame="frame_n")


def report(key, value):
    REPORT[key] = value
    out = os.environ.get("WLK_REPORT_DIR") or os.path.join(ROOT, "test_reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "head_survey_report.json"), "w") as fh:
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
    """one wlk_diag_head_survey call on a case; keeps what was sent"""

    def __init__(self, c, k_splits=0, **override):
        self.c = c
        self.n = c["n_layer"] * c["n_head"] * c["P"]
        self.buf = dict(q=guarded(c["q"]), k=guarded(c["k"]), peak=guard(self.n + TAIL), frame=np.full(self.n + TAIL, IGUARD, np.int32))
        kw = dict(n_layer=c["n_layer"], n_head=c["n_head"], P=c["P"], F=c["F"], Tk=c["Tk"], k_splits=k_splits, ldq=c["ldq"], ldkv=c["ldkv"])
        sizes = {}
        for key in list(override):
            if key in POINTERS:
                self.buf[key] = override.pop(key)
            elif key in SIZES.values():
                sizes[key] = override.pop(key)
        kw.update(override)
        self.sent = {key: None if v is None else v.copy() for key, v in self.buf.items()}
        args = _lib.DiagHeadSurveyArgs()
        for key, v in self.buf.items():
            if v is not None:
                setattr(args, key, v.ctypes.data)
                setattr(args, SIZES[key], v.size)
        for key, val in {**kw, **sizes}.items():
            setattr(args, key, val)
        lib = _lib.load()
        self.rc = lib.wlk_diag_head_survey(C.byref(args))
        self.msg = "" if self.rc == 0 else lib.wlk_diag_last_error().decode()
        if self.rc not in (0, WLK_ERR_ARG):     # a HIP error: the device's state is unknown, nothing more is launched on it
            pytest.exit(f"wlk_diag_head_survey ({c['name']}): error {self.rc}: {self.msg}", returncode=3)

    def unchanged(self, keys=POINTERS):
        return [k for k in keys if self.sent[k] is not None and not np.array_equal(bits(self.buf[k]), bits(self.sent[k]))]

    def words(self):
        """-> failures: an input changed, a word behind a result written, an owned word that still holds the guard"""
        fails = [f"changed its input {k}" for k in self.unchanged(("q", "k"))]
        for key in ("peak", "frame"):
            now, sent = bits(self.buf[key]), bits(self.sent[key])
            if not np.array_equal(now[self.n:], sent[self.n:]):
                fails.append(f"wrote {int((now[self.n:] != sent[self.n:]).sum())} words of {key} it does not own")
            if (now[:self.n] == sent[:self.n]).any():
                fails.append(f"left {int((now[:self.n] == sent[:self.n]).sum())} owned words of {key} unwritten")
        return fails

    def got(self):
        shape = (self.c["n_layer"], self.c["n_head"], self.c["P"])
        return self.buf["peak"][:self.n].reshape(shape).copy(), self.buf["frame"][:self.n].reshape(shape).copy()


def check_values(ref, peak, frame, what):
    """-> (failures, figures) of one result against the float64 statement"""
    fails = []
    tol, e32 = SR.value_tolerance(ref=ref["denom64"], f32=ref["denom32"])
    with np.errstate(divide="ignore"):
        denom = 1.0 / peak.astype(np.float64)
    err = SR.abs_err(denom, ref["denom64"])
    if not (err <= tol).all():
        at = np.unravel_index(int((err - tol).argmax()), err.shape)
        fails.append(f"{what}: 1/peak off by {err[at]:.3e} at {at} (allowed {tol[at]:.3e}, reference {ref['denom64'][at]:.6g})")
    wrong = np.argwhere(frame != ref["frame64"])
    if len(wrong):
        at = tuple(wrong[0])
        fails.append(f"{what}: {len(wrong)} frames differ from the float64 arg-max, first at {at}: {frame[at]} for {ref['frame64'][at]}")
    return fails, dict(err_max=float(err.max()), e32=e32, rel_err_max=float((err / ref["denom64"]).max()), tol_min=float(tol.min()))


@pytest.mark.parametrize("name", HC.NAMES)
def test_kernel_against_float64_every_key_split(name):
    c, ref = HC.case(name), HC.reference(name)
    fails, rep, got = [], {}, {}
    splits = sorted({0, 1, 2, HC.max_splits(c["F"])})
    for ks in splits:
        run = Run(c, ks)
        assert run.rc == 0, run.msg
        fails += [f"split {ks}: {f}" for f in run.words()]
        got[ks] = run.got()
        f, r = check_values(ref, *got[ks], what=f"split {ks}")
        fails += f
        rep[f"split{ks}"] = r
    print(name, json.dumps(rep))
    report(name, rep)
    for ks in splits:
        if not np.array_equal(got[ks][1], got[1][1]):
            fails.append(f"split {ks} gives other frames than split 1")
    for p in c["equal_rows"]:
        for ks in splits:
            if not (got[ks][1][:, :, p] == 0).all() or not np.array_equal(got[ks][0][:, :, p], np.full_like(got[ks][0][:, :, p], np.float32(1) / np.float32(c["F"]))):
                fails.append(f"split {ks}: the all-equal row {p} is not (1 / F, frame 0)")
    for p, where in c["ties"]:
        for ks in splits:
            if not (got[ks][1][:, :, p] == min(where)).all():
                fails.append(f"split {ks}: tie row {p} over keys {where} returned {np.unique(got[ks][1][:, :, p]).tolist()}")
    again = Run(c, splits[-1]).got()
    if not np.array_equal(bits(again[0]), bits(got[splits[-1]][0])) or not np.array_equal(again[1], got[splits[-1]][1]):
        fails.append("a second launch gives another result")
    assert not fails, "\n".join(fails)


def test_kernel_without_frames_and_with_a_clamped_split():
    c, ref = HC.case("f129_p31_h1_l1_tk129"), HC.reference("f129_p31_h1_l1_tk129")
    base = Run(c, HC.max_splits(c["F"]))
    run = Run(c, 1000, frame=None)          # more ranges than 128-key trips: clamped to their count
    assert run.rc == 0, run.msg
    assert np.array_equal(bits(run.buf["peak"]), bits(base.buf["peak"]))
    assert not run.unchanged(("q", "k"))


def test_refusals_of_the_launcher_and_of_the_buffers():
    c = HC.case("f3_p31_h2_l3_tk8")
    L, H, P, Tk, d = c["n_layer"], c["n_head"], c["P"], c["Tk"], 64 * c["n_head"]
    cases = [
        (dict(F=0), "P, F, Tk in [1, 2^20]"),
        (dict(P=0), "P, F, Tk in [1, 2^20]"),
        (dict(n_head=0), "n_layer, n_head in [1, 256]"),
        (dict(n_layer=257), "n_layer, n_head in [1, 256]"),
        (dict(F=Tk + 1), "F beyond the Tk key rows"),
        (dict(k_splits=-1), "negative key split"),
        (dict(ldkv=c["ldkv"] - 4), "key rows shorter than"),
        (dict(ldq=d - 4), "query rows at least 64 n_head floats apart"),
        (dict(ldq=d + 2), "a multiple of 4"),
        (dict(peak=None), "null q, k or peak"),
        (dict(q_floats=(L * P - 1) * c["ldq"] + d - 1), "the query rows lie past q"),
        (dict(k_floats=(Tk - 1) * c["ldkv"] + (L - 1) * 2 * d + d - 1), "the Tk key rows lie past k"),
        (dict(peak_floats=L * H * P - 1), "peak holds fewer"),
        (dict(frame_n=L * H * P - 1), "frame holds fewer"),
    ]
    for override, text in cases:
        run = Run(c, override.pop("k_splits", 0), **override)
        assert run.rc == WLK_ERR_ARG and text in run.msg, (override, run.rc, run.msg)
        assert not run.unchanged(), (override, "a refused call changed a buffer")
    assert _lib.load().wlk_diag_head_survey(None) == WLK_ERR_ARG


# ---- through the model ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    from whisperlivekit_amd.engine import HipWhisperModel
    dims, sd = HC.planted_state_dict()
    model = HipWhisperModel.from_state_dict(dims, sd, [(1, 0), (1, 1)], device=0)
    yield dims, sd, model
    model.close()


def softmax_fold(s):
    """float64 scores [..., F] -> (denom, frame)"""
    s = np.asarray(s, np.float64)
    return np.exp(s - s.max(-1, keepdims=True)).sum(-1), s.argmax(-1)


@pytest.mark.parametrize("P,num_frames", [(3, 3000), (14, 3000), (40, 3000), (14, 1000), (40, 1001)])
def test_survey_against_the_debug_export_and_the_oracle(planted, P, num_frames):
    import torch
    dims, sd, model = planted
    L, H, F = dims.n_text_layer, dims.n_text_head, num_frames // 2
    mel, tokens = HC.planted_mel(7), HC.planted_tokens(7, P)
    s_or, _ = HC.oracle_peaks(sd, dims, mel, tokens, num_frames, dtype=torch.float64)
    denom_or, _ = softmax_fold(s_or)
    a, b = model.new_session(beam=1, batched=False), model.new_session(beam=1, batched=False)
    try:
        a.encode_mel(mel)
        peaks, frames = a.head_survey(tokens, num_frames)
        b.set_debug(True)
        b.encode_mel(mel)
        b.decode(tokens[None], first=True)
        s_b = np.stack([b.export(f"cross_qk:{l}").reshape(P, H, 1500).transpose(1, 0, 2) for l in range(L)])[..., :F]
    finally:
        a.close()
        b.close()
    assert peaks.shape == frames.shape == (L, H, P) and peaks.dtype == np.float32 and frames.dtype == np.int32
    denom_b, _ = softmax_fold(s_b)
    err_b = float(np.abs(denom_b - denom_or).max())
    score_err_b = float(np.abs(s_b.astype(np.float64) - s_or).max())
    err_a = np.abs(1.0 / peaks.astype(np.float64) - denom_or)
    tol = np.maximum(SR.KERNEL_FACTOR * err_b, SR.FLOOR * denom_or)
    assert (frames >= 0).all() and (frames < F).all()
    behind = s_or.max(-1) - np.take_along_axis(s_or, frames[..., None].astype(np.int64), -1)[..., 0]
    rep = dict(err_survey=float(err_a.max()), err_debug_export=err_b, score_err_debug_export=score_err_b,
               frame_behind_max=float(behind.max()), denom_max=float(denom_or.max()))
    print(P, num_frames, json.dumps(rep))
    report(f"model_p{P}_frames{num_frames}", rep)
    assert (err_a <= tol).all(), rep
    assert (behind <= score_err_b).all(), rep


def test_session_state_after_a_survey(planted):
    dims, sd, model = planted
    mel, tokens = HC.planted_mel(8), HC.planted_tokens(8, 20)
    prompt = np.array([[50258, 50259, 50359, 50363]], np.int64)

    def decode_some(s):
        out = []
        feed = prompt
        for step in range(3):
            s.decode(feed, first=(step == 0), sot_index=0)
            logits = s.export("logits_last").reshape(-1).copy()
            out.append(logits)
            feed = np.array([[int(logits.argmax())]], np.int64)
        return out

    a, fresh = model.new_session(beam=1, batched=False), model.new_session(beam=1, batched=False)
    try:
        a.encode_mel(mel)
        fresh.encode_mel(mel)
        one = a.head_survey(tokens)
        two = a.head_survey(tokens)
        assert np.array_equal(bits(one[0]), bits(two[0])) and np.array_equal(one[1], two[1])
        with pytest.raises(_lib.WlkError) as e:      # the window holds nothing a step could continue
            a.decode(np.array([[100]], np.int64), first=False)
        assert e.value.code == WLK_ERR_STATE
        want = decode_some(fresh)
        for x, y in zip(decode_some(a), want):
            assert np.array_equal(bits(x), bits(y))
        three = a.head_survey(tokens)               # and after ordinary decoding the survey repeats itself
        assert np.array_equal(bits(one[0]), bits(three[0])) and np.array_equal(one[1], three[1])
    finally:
        a.close()
        fresh.close()
    # the survey reads no head table: the same weights without alignment heads
    from whisperlivekit_amd.engine import HipWhisperModel
    bare = HipWhisperModel.from_state_dict(dims, sd, [], device=0)
    try:
        assert bare.alignment_heads == []
        s = bare.new_session(beam=1, batched=False)
        try:
            s.encode_mel(mel)
            none = s.head_survey(tokens)
        finally:
            s.close()
    finally:
        bare.close()
    assert np.array_equal(bits(one[0]), bits(none[0])) and np.array_equal(one[1], none[1])


def test_refusals_of_head_survey(planted):
    dims, sd, model = planted
    lib = _lib.load()
    L, H = dims.n_text_layer, dims.n_text_head
    mel = HC.planted_mel(9)
    good = HC.planted_tokens(9, 6)

    def call(s, tokens, num_frames=3000, peak=True, n=None, handle=True):
        toks = np.ascontiguousarray(tokens, np.int64)
        n = len(toks) if n is None else n
        out = np.empty(L * H * max(n, 1), np.float32)
        rc = lib.wlk_head_survey(s._h if handle else None, toks.ctypes.data_as(C.POINTER(C.c_int64)) if tokens is not None else None, n,
                                 num_frames, out.ctypes.data_as(C.POINTER(C.c_float)) if peak else None, None)
        return rc, (lib.wlk_last_error() or b"").decode()

    sess, beam2 = model.new_session(beam=1, batched=False), model.new_session(beam=2, batched=False)
    attached, debug, prof = (model.new_session(beam=1, batched=False) for _ in range(3))
    try:
        rc, msg = call(sess, good)
        assert rc == WLK_ERR_STATE and "before an encode" in msg, (rc, msg)
        for s in (sess, beam2, attached, debug, prof):
            s.encode_mel(mel)
        attached.attach_engine()
        debug.set_debug(True)
        prof.prof_begin()
        for kw, code, text in [
                (dict(s=sess, tokens=good, handle=False), WLK_ERR_ARG, "NULL argument"),
                (dict(s=sess, tokens=good, peak=False), WLK_ERR_ARG, "NULL argument"),
                (dict(s=beam2, tokens=good), WLK_ERR_ARG, "beam-1 session"),
                (dict(s=sess, tokens=good, n=0), WLK_ERR_ARG, "n_tokens must be >= 1"),
                (dict(s=sess, tokens=good, num_frames=1), WLK_ERR_ARG, "num_frames out of range"),
                (dict(s=sess, tokens=good, num_frames=2 * dims.n_audio_ctx + 2), WLK_ERR_ARG, "num_frames out of range"),
                (dict(s=sess, tokens=np.full(dims.n_text_ctx + 1, 100)), WLK_ERR_CAPACITY, "more tokens than the text context"),
                (dict(s=sess, tokens=[100, dims.n_vocab, 5]), WLK_ERR_ARG, "token id out of range"),
                (dict(s=sess, tokens=[100, -1, 5]), WLK_ERR_ARG, "token id out of range"),
                (dict(s=attached, tokens=good), WLK_ERR_STATE, "attached to the batch engine"),
                (dict(s=debug, tokens=good), WLK_ERR_STATE, "debug or profiling"),
                (dict(s=prof, tokens=good), WLK_ERR_STATE, "debug or profiling")]:
            rc, msg = call(**kw)
            assert rc == code and text in msg, (kw.get("tokens"), rc, msg)
        prof.prof_end()
        rc, msg = call(sess, good)                  # and the session still surveys afterwards
        assert rc == 0, msg
        peaks, _ = sess.head_survey(np.full(dims.n_text_ctx, 100), 3000)       # the longest row the context holds
        assert np.isfinite(peaks).all() and (peaks > 0).all() and (peaks <= 1).all()
    finally:
        for s in (sess, beam2, attached, debug, prof):
            s.close()


def test_planted_heads_end_to_end(planted):
    from whisperlivekit_amd.backend import HipSimulStreamingASR
    dims, sd, model = planted
    counts = {}
    clips = [HC.planted_clip(seed) for seed in range(3)] + [(HC.planted_clip(0)[0], "clip 0")]
    votes, strengths = AH.collect_heads(model, HC.PlantedTokenizer, clips[:3], counts=counts)
    print(strengths.tolist(), votes.tolist())
    report("planted", dict(strengths=strengths.tolist(), votes=votes.tolist()))
    assert counts == dict(used=3, skipped=0)
    mask = AH.select_heads(strengths, votes)
    assert AH.mask_pairs(mask) == sorted(HC.PLANTED)
    asr = HipSimulStreamingASR("micro", state_dict=sd, custom_alignment_heads=AH.dump_mask(mask))
    try:
        assert asr.hip_model.alignment_heads == sorted(HC.PLANTED)
    finally:
        asr.hip_model.close()

    class Long(HC.PlantedTokenizer):
        @staticmethod
        def encode(text):
            return [100] * (dims.n_text_ctx if text == "long" else 3)

    counts = {}
    AH.collect_heads(model, Long, [(clips[0][0], "long"), (clips[0][0], "short")], counts=counts)
    assert counts == dict(used=1, skipped=1)
    with pytest.raises(ValueError):
        AH.collect_heads(model, Long, [(clips[0][0], "long")])


def test_command_line(tmp_path):
    import torch
    dims, sd = HC.planted_state_dict()
    ckpt = tmp_path / "planted.pt"
    import dataclasses
    torch.save({"dims": dataclasses.asdict(dims),
                "model_state_dict": {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}}, str(ckpt))
    lines = []
    for seed in range(2):
        audio, _ = HC.planted_clip(seed)
        np.save(str(tmp_path / f"clip{seed}.npy"), audio.astype(np.float32))
        lines.append(json.dumps(dict(audio=f"clip{seed}.npy", text=HC.CLI_TEXT)))
    (tmp_path / "clips.jsonl").write_text("\n".join(lines) + "\n")
    out = tmp_path / "heads.b85"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), WLK_SYNTHETIC_VOCAB="1")
    done = subprocess.run([sys.executable, "-m", "whisperlivekit_amd.alignment_heads", "--model", str(ckpt), "--clips",
                           str(tmp_path / "clips.jsonl"), "--output", str(out)], cwd=ROOT, env=env, capture_output=True, text=True,
                          timeout=300)
    print(done.stdout, done.stderr[-2000:])
    assert done.returncode == 0, done.stderr[-2000:]
    mask = AH.load_mask(out.read_text(), dims)
    assert AH.mask_pairs(mask) == sorted(HC.PLANTED)
    assert "pairs: 0,1 1,0" in done.stdout and "layer  0:" in done.stdout
