"""Stacked word alignment on the GPU (csrc/window_group.hip: wlk_group_find_alignment, csrc/dtw.hip: the
ragged recurrence and dtw_walk_kernel, csrc/word_align.hip: the ragged normalisation).

  dtw_starts      the ragged warping launches on host matrices (wlk_diag_dtw_starts): every step code is
                  timing_oracle.dtw_trace's, the starts are those of timing_oracle.backtrace - integers, no tolerance;
                  eight matrices of different shapes in one call give each the bits of a call of one.
  with a model    tiny.en with seeded weights (the smallest model the stacked chain takes): a window's starts,
                  probabilities, cost and trace do not depend on the windows beside it, cost and probabilities are the solo
                  wlk_find_alignment's bits, one case against the float64 oracle, refusals launch nothing and touch nobody,
                  the sessions afterwards, and `transcribe` with the switch on and off.
Every output buffer carries guard words behind it; no owned word may be left holding the guard."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import helpers as H
import align_stack_cases as AC
from oracle import timing_oracle
from whisperlivekit_amd import _lib, synth, timing, transcribe as TR
from whisperlivekit_amd.dims import ALIGNMENT_HEADS, MODEL_DIMS

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
from gen_golden_dtw import dtw_case_matrix  # noqa: E402

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -3
TAIL = 64
FGUARD = np.uint32(0x7FC12345)           # a NaN with a payload: reading it poisons, and it is recognisable
IGUARD, BGUARD = np.int32(-77777), np.int8(0x55)
vp = lambda a: a.ctypes.data_as(C.c_void_p)        # noqa: E731


def fguard(n):
    return np.full(n, FGUARD, np.uint32).view(np.float32)


def is_fguard(a):
    return a.view(np.uint32) == FGUARD


# ---- GPU, no model: the ragged recurrence + path walk ------------------------------------------------------------------------------
def dtw_starts(mats):
    """wlk_diag_dtw_starts on the matrices, twice (the second call repeats the first); checks the guards, that no owned
    word is left unwritten and that the input is untouched.  -> [(starts, trace)] per matrix"""
    lib = _lib.load()
    sizes = [m.size for m in mats]
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    costs = np.concatenate([np.ascontiguousarray(m, np.float32).reshape(-1) for m in mats] + [fguard(TAIL)])
    before = costs.copy()
    nr = np.array([m.shape[0] for m in mats], np.int32)
    nc = np.array([m.shape[1] for m in mats], np.int32)
    n_s, n_t = int(nr.sum()), int(((nr + 1) * (nc + 1)).sum())
    runs = []
    for _ in range(2):
        starts = np.full(n_s + TAIL, IGUARD, np.int32)
        traces = np.full(n_t + TAIL, BGUARD, np.int8)
        _lib.check(lib.wlk_diag_dtw_starts(vp(costs), vp(offsets), vp(nr), vp(nc), len(mats), vp(starts), vp(traces)))
        assert (starts[n_s:] == IGUARD).all() and (traces[n_t:] == BGUARD).all(), "a guard word behind a result was written"
        assert not (starts[:n_s] == IGUARD).any() and not (traces[:n_t] == BGUARD).any(), "an owned word was left unwritten"
        assert np.array_equal(costs.view(np.uint32), before.view(np.uint32)), "the input changed"
        runs.append((starts, traces))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]), "a second call differs"
    out, at_s, at_t = [], 0, 0
    for m in mats:
        n, k = m.shape
        out.append((runs[0][0][at_s:at_s + n].copy(), runs[0][1][at_t:at_t + (n + 1) * (k + 1)].reshape(n + 1, k + 1).copy()))
        at_s, at_t = at_s + n, at_t + (n + 1) * (k + 1)
    return out


KAT = H.golden_npz("dtw_kat.npz")
SHAPES = [(1, 1), (1, 70), (65, 1), (254, 5)] + [(n, m) for n in (63, 64, 65) for m in (63, 64, 65, 128, 129)]
DTW_CASES = [(f"plain_{n}x{m}", "plain", n, m, 7 * n + m) for n, m in SHAPES] + [("largest_254x1500", "plain", 254, 1500, 3)] + [
    (f"{kind}_{n}x{m}", kind, n, m, n + m) for kind in ("nan_row", "inf_col", "ties", "quant") for n, m in ((65, 129), (40, 200))] + [
    (f"kat_{n}", f"kat:{k}", *map(int, s)) for n, k, s in zip(KAT["names"], KAT["kinds"], KAT["shapes"])]


def case_matrix(kind, n, m, seed):
    return dtw_case_matrix(kind[4:], n, m, seed) if kind.startswith("kat:") else AC.cost_matrix(kind, n, m, seed)


_ORACLE = {}


def oracle(name, x):
    """the reference trace and starts of a case, computed once and shared"""
    if name not in _ORACLE:
        trace = timing_oracle.dtw_trace(x)
        _ORACLE[name] = (trace, AC.starts_of_trace(trace))
    return _ORACLE[name]


@pytest.mark.parametrize("name,kind,n,m,seed", DTW_CASES, ids=[c[0] for c in DTW_CASES])
def test_dtw_starts(name, kind, n, m, seed):
    x = case_matrix(kind, n, m, seed)
    (starts, trace), = dtw_starts([x])
    want_trace, want_starts = oracle(name, x)
    np.testing.assert_array_equal(trace, want_trace)
    np.testing.assert_array_equal(starts, want_starts)
    if kind.startswith("kat:"):
        np.testing.assert_array_equal(starts, AC.starts_of_path(KAT[f"path_{name[4:]}"], n))


def test_dtw_starts_of_eight_ragged_matrices_in_one_call():
    picks = ["plain_1x1", "plain_65x1", "plain_1x70", "plain_64x129", "nan_row_65x129", "ties_40x200", "kat_window_30s",
             "plain_254x5"]
    cases = {c[0]: c for c in DTW_CASES}
    order = np.random.default_rng(5).permutation(len(picks))
    mats = [case_matrix(*cases[picks[i]][1:]) for i in order]
    assert len({m.shape for m in mats}) == 8
    got = dtw_starts(mats)
    for i, x, (starts, trace) in zip(order, mats, got):
        (s1, t1), = dtw_starts([x])
        assert np.array_equal(starts, s1) and np.array_equal(trace, t1), f"{picks[i]}: differs from the call of one"
        want_trace, want_starts = oracle(picks[i], x)
        assert np.array_equal(trace, want_trace) and np.array_equal(starts, want_starts), picks[i]


# ---- GPU, with a model ---------------------------------------------------------------------------------------------------------------
NAME, SEED = "tiny.en", 3
SOT, NO_TS, EOT = [50257], 50362, 50256
WINDOWS = [(9, 10), (32, 1511), (33, 3000), (64, 10), (100, 1511), (256, 3000), (9, 3000), (256, 10)]     # (P, num_frames)


def window_tokens(k):
    p = WINDOWS[k][0]
    text = np.random.default_rng(100 + k).integers(0, EOT, p - len(SOT) - 2).tolist()
    return [*SOT, NO_TS, *text, EOT]


class Call:
    """One wlk_group_find_alignment call with guarded output buffers."""

    def __init__(self, group, wins, want=True):
        """wins: (session, tokens, num_frames) each"""
        self.n = len(wins)
        self.arr = (_lib.AlignWindow * max(self.n, 1))()
        self.bufs, self.keep = [], []
        for a, (sess, tokens, nf) in zip(self.arr, wins):
            toks = np.ascontiguousarray(tokens, dtype=np.int64)
            n_text, f = max(len(toks) - len(SOT) - 2, 1), max(nf // 2, 1)
            b = dict(n_text=n_text, f=f, starts=np.full(n_text + 1 + TAIL, IGUARD, np.int32), probs=fguard(n_text + TAIL),
                     cost=fguard((n_text + 1) * f + TAIL), trace=np.full((n_text + 2) * (f + 1) + TAIL, BGUARD, np.int8))
            a.s, a.tokens, a.n_tokens, a.n_sot, a.eot, a.num_frames, a.qk_scale = sess._h, vp(toks).value, len(toks), len(SOT), EOT, nf, 1.0
            a.starts, a.token_probs = vp(b["starts"]).value, vp(b["probs"]).value
            a.cost, a.trace = (vp(b["cost"]).value, vp(b["trace"]).value) if want else (None, None)
            self.keep.append(toks)
            self.bufs.append(b)
        self.rc = group.lib.wlk_group_find_alignment(group._h, self.arr, self.n)

    def untouched(self):
        return all((b["starts"] == IGUARD).all() and is_fguard(b["probs"]).all() and is_fguard(b["cost"]).all()
                   and (b["trace"] == BGUARD).all() for b in self.bufs)

    def results(self):
        """-> [dict(starts, probs, cost, trace)]; checks the guards and that every owned word was written"""
        assert self.rc == 0, _lib.load().wlk_last_error()
        out = []
        for b in self.bufs:
            nt, f = b["n_text"], b["f"]
            own = dict(starts=b["starts"][:nt + 1], probs=b["probs"][:nt], cost=b["cost"][:(nt + 1) * f],
                       trace=b["trace"][:(nt + 2) * (f + 1)])
            assert (b["starts"][nt + 1:] == IGUARD).all() and is_fguard(b["probs"][nt:]).all(), "a guard word was written"
            assert is_fguard(b["cost"][(nt + 1) * f:]).all() and (b["trace"][(nt + 2) * (f + 1):] == BGUARD).all(), "a guard word was written"
            assert not (own["starts"] == IGUARD).any() and not is_fguard(own["probs"]).any(), "an owned word was left unwritten"
            assert not is_fguard(own["cost"]).any() and not (own["trace"] == BGUARD).any(), "an owned word was left unwritten"
            out.append(dict(starts=own["starts"].copy(), probs=own["probs"].copy(), cost=own["cost"].reshape(nt + 1, f).copy(),
                            trace=own["trace"].reshape(nt + 2, f + 1).copy()))
        return out


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in ("starts", "probs", "cost", "trace"))


@pytest.fixture(scope="module")
def rig():
    """tiny.en, a group of 8, one encoded session per window (each its own speech-like mel) and every window's result in
    a group of one: the reference of the stacked runs, computed once"""
    from whisperlivekit_amd.engine import HipWhisperModel, HipWindowGroup
    model = HipWhisperModel.synthetic(NAME, SEED, device=0)
    group = HipWindowGroup(model, 8)
    sessions, mels = [], []
    for k in range(len(WINDOWS)):
        s = model.new_session(beam=1, max_audio_seconds=31.0, batched=False)
        mel = TR.pad_or_trim(s.log_mel(synth.speech_like(6.0 + 3 * k, seed=40 + k)))
        s.encode_mel(mel)
        sessions.append(s)
        mels.append(mel)
    wins = [(sessions[k], window_tokens(k), WINDOWS[k][1]) for k in range(len(WINDOWS))]
    single = [Call(group, [w]).results()[0] for w in wins]
    yield dict(model=model, group=group, sessions=sessions, mels=mels, wins=wins, single=single)
    for s in sessions:
        s.close()
    group.close()
    model.close()


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
def test_a_window_does_not_depend_on_the_windows_beside_it(n, rig):
    order = np.random.default_rng(n).permutation(len(WINDOWS))[:n]
    got = Call(rig["group"], [rig["wins"][k] for k in order]).results()
    bad = [f"window {k} {WINDOWS[k]}" for k, g in zip(order, got) if not same_bits(g, rig["single"][k])]
    assert not bad, f"stack of {n}: not the bits of the group of one: {bad}"
    # the product path asks for neither cost nor trace: same starts and probabilities
    lean = Call(rig["group"], [rig["wins"][k] for k in order], want=False)
    assert lean.rc == 0
    for k, b in zip(order, lean.bufs):
        assert np.array_equal(b["starts"][:b["n_text"] + 1], rig["single"][k]["starts"])
        assert np.array_equal(b["probs"][:b["n_text"]].view(np.uint32), rig["single"][k]["probs"].view(np.uint32))
        assert is_fguard(b["cost"]).all() and (b["trace"] == BGUARD).all()


def test_the_group_against_the_solo_call(rig):
    """cost and token probabilities are wlk_find_alignment's bits (a stacked row goes through its session's own
    arithmetic); the starts are those of timing.backtrace of the solo trace."""
    bad = []
    for k, (sess, tokens, nf) in enumerate(rig["wins"]):
        trace, probs, cost = sess.find_alignment(tokens, len(SOT), EOT, nf, want_cost=True)
        g = rig["single"][k]
        if not np.array_equal(cost.view(np.uint32), g["cost"].view(np.uint32)):
            bad.append(f"window {k} {WINDOWS[k]}: cost differs in {int((cost.view(np.uint32) != g['cost'].view(np.uint32)).sum())} cells, "
                       f"max {float(np.nanmax(np.abs(cost - g['cost']))):.3e}")
        if not np.array_equal(probs.view(np.uint32), g["probs"].view(np.uint32)):
            bad.append(f"window {k} {WINDOWS[k]}: token probabilities differ, max {float(np.abs(probs - g['probs']).max()):.3e}")
        if not np.array_equal(g["starts"], AC.starts_of_path(timing.backtrace(trace), len(tokens) - len(SOT) - 1)):
            bad.append(f"window {k} {WINDOWS[k]}: starts differ from backtrace of the solo trace")
        if not np.array_equal(trace, g["trace"]):
            bad.append(f"window {k} {WINDOWS[k]}: trace differs")
    assert not bad, "\n".join(bad)


def test_the_group_against_float64(rig):
    """P = 100, num_frames = 1511 (window 4) stacked beside two others: the cost within 4 x the float32 oracle's own error
    (floor 2e-5), probabilities at rtol 2e-4 - the rules of tests/test_word_timing.py; the path only as the DTW of the
    kernel's own cost (a discrete path may legitimately differ under fp32 error)."""
    import torch
    from select_reference import abs_err
    k = 4
    assert WINDOWS[k] == (100, 1511)
    dims, heads = MODEL_DIMS[NAME], ALIGNMENT_HEADS[NAME]
    sd32 = H.oracle_sd(NAME, SEED)
    sd64 = {n: v.double() if v.is_floating_point() else v for n, v in sd32.items()}
    mel = torch.from_numpy(np.ascontiguousarray(rig["mels"][k]))
    text = window_tokens(k)[len(SOT) + 1:-1]
    want, probs64 = timing_oracle.alignment_cost(sd64, dims, heads, mel.double(), SOT, NO_TS, text, EOT, 1511, dtype=np.float64)
    f32, _ = timing_oracle.alignment_cost(sd32, dims, heads, mel, SOT, NO_TS, text, EOT, 1511)
    got = Call(rig["group"], [rig["wins"][2], rig["wins"][k], rig["wins"][7]]).results()[1]
    assert got["cost"].shape == want.shape == (98, 755)
    e32, err = float(abs_err(f32, want).max()), float(abs_err(got["cost"], want).max())
    allowed = max(4 * e32, 2e-5)
    perr = float(np.max(np.abs(got["probs"] - np.asarray(probs64)) / np.maximum(np.abs(probs64), 1e-30)))
    print(f"\nP 100 num_frames 1511: cost error {err:.3e}, float32 oracle {e32:.3e}, allowed {allowed:.3e}; "
          f"probabilities: worst relative error {perr:.3e}")
    assert err <= allowed
    np.testing.assert_allclose(got["probs"], probs64, rtol=2e-4, atol=1e-9)
    trace = timing_oracle.dtw_trace(got["cost"])
    assert np.array_equal(got["trace"], trace) and np.array_equal(got["starts"], AC.starts_of_trace(trace))


def test_refusals_launch_nothing_and_touch_nobody(rig):
    from whisperlivekit_amd.engine import HipWhisperModel
    model, group, wins = rig["model"], rig["group"], rig["wins"]
    other = HipWhisperModel.synthetic(NAME, SEED + 1, device=0)
    foreign = other.new_session(beam=1, max_audio_seconds=31.0, batched=False)
    fresh = model.new_session(beam=1, max_audio_seconds=31.0, batched=False)
    attached = model.new_session(beam=1, max_audio_seconds=31.0, batched=True)
    try:
        foreign.encode_mel(rig["mels"][0])
        attached.encode_mel(rig["mels"][0])
        tok = lambda p: [*SOT, NO_TS, *range(1, p - 2), EOT]                     # noqa: E731
        s0 = wins[0][0]
        refused = [
            ("a session twice", [wins[1], wins[2], (wins[1][0], tok(20), 3000)], ERR_ARG),
            ("a session of another model", [wins[1], (foreign, tok(20), 3000), wins[2]], ERR_ARG),
            ("an unencoded session", [wins[1], wins[2], (fresh, tok(20), 3000)], ERR_STATE),
            ("an engine-attached session", [(attached, tok(20), 3000), wins[1], wins[2]], ERR_STATE),
            ("P = 8", [wins[1], wins[2], (s0, tok(8), 3000)], ERR_ARG),
            ("P = 257", [wins[1], (s0, tok(257), 3000), wins[2]], ERR_ARG),
            ("no frames", [wins[1], wins[2], (s0, tok(20), 1)], ERR_ARG),
            ("frames beyond the encoder", [wins[1], wins[2], (s0, tok(20), 3002)], ERR_ARG),
            ("a text token >= eot", [wins[1], wins[2], (s0, [*SOT, NO_TS, 5, EOT, 6, 7, 8, 9, 10, EOT], 3000)], ERR_ARG),
            ("n = 0", [], ERR_ARG),
            ("n = 9", wins + [(fresh, tok(20), 3000)], ERR_ARG),
        ]
        for what, call_wins, code in refused:
            c = Call(group, call_wins)
            assert c.rc == code, f"{what}: returned {c.rc}, not {code}"
            assert c.untouched(), f"{what}: an output was written"
            # the others then give the bits of a twin that never met the refused call
            got = Call(group, [wins[1], wins[2]]).results()
            assert same_bits(got[0], rig["single"][1]) and same_bits(got[1], rig["single"][2]), what
        for p, nf, want in ((8, 3000, False), (9, 3000, True), (256, 10, True), (257, 3000, False), (100, 1, False),
                            (100, 2, True), (100, 3001, True), (100, 3002, False)):
            assert group.fits(p, nf) is want, (p, nf)
            c = Call(group, [(s0, tok(p), nf)])
            assert (c.rc == 0) is want, (p, nf, c.rc)
            assert want or c.untouched()
        # a model narrower than 256 never fits: the k-wave GEMMs need K >= 256
        from whisperlivekit_amd.engine import HipWindowGroup
        micro = HipWhisperModel.synthetic("micro.en", 0, device=0)
        try:
            g2 = HipWindowGroup(micro, 4)
            assert not any(g2.fits(p, 3000) for p in (9, 32, 100, 256))
            g2.close()
        finally:
            micro.close()
    finally:
        for s in (foreign, fresh, attached):
            s.close()
        other.close()


def test_the_sessions_afterwards(rig):
    sess, tokens, nf = rig["wins"][3]
    Call(rig["group"], [rig["wins"][3], rig["wins"][0]]).results()
    with pytest.raises(_lib.WlkError, match="first decode of an infer must set first=1"):
        sess.decode(np.array([[1000]]), first=False)
    # a fresh encode + prefill + read-out, then the window again: the group of one's bits
    sess.append(np.zeros(16000, np.float32))
    sess.encode()
    sess.decode(np.array([[50257, 50362, 1000]]), first=True, sot_index=0)
    sess.select([], [], [], 2, 50)
    sess.encode_mel(rig["mels"][3])
    assert same_bits(Call(rig["group"], [rig["wins"][3]]).results()[0], rig["single"][3])


def test_transcribe_with_the_switch_equals_transcribe_without(tmp_path, monkeypatch):
    from whisperlivekit_amd.engine import HipWhisperModel
    monkeypatch.setenv("WLK_VOCAB_DIR", H.real_vocab_dir(tmp_path))
    monkeypatch.setenv("WLK_SYNTHETIC_VOCAB", "0")
    monkeypatch.delenv("WLK_TRANSCRIBE_ALIGN_STACK", raising=False)
    monkeypatch.setenv("WLK_TRANSCRIBE_STACK", "3")
    model = HipWhisperModel.synthetic(NAME, SEED, device=0)
    kw = dict(language="en", word_timestamps=True, temperature=0.0, logprob_threshold=None, compression_ratio_threshold=None,
              sample_len=40, without_timestamps=True)       # text up to sample_len: windows long enough for the stack
    audios = [synth.speech_like(sec, seed=60 + i) for i, sec in enumerate((5.0, 8.0, 11.0))]
    aligned = []
    solo = timing.find_alignment

    def counting(session, tokenizer, text_tokens, mel, num_frames, **k):
        if len(text_tokens):
            aligned.append((mel is None, len(tokenizer.sot_sequence) + 2 + len(text_tokens), num_frames))
        return solo(session, tokenizer, text_tokens, mel, num_frames, **k)
    monkeypatch.setattr(timing, "find_alignment", counting)
    try:
        want = TR.transcribe_many(model, audios, stack=3, **kw)
        assert TR.align_stacker(model) is None and len(aligned) >= 3 and all(a[0] for a in aligned)
        assert sum(len(seg["words"]) for r in want for seg in r["segments"]) > 0
        fit = [TR.window_stacker(model).group.fits(p, nf) for _held, p, nf in aligned]
        assert sum(fit) >= 3, aligned
        del aligned[:]
        monkeypatch.setenv("WLK_TRANSCRIBE_ALIGN_STACK", "1")
        got = TR.transcribe_many(model, audios, stack=3, **kw)
        assert got == want
        st = TR.align_stacker(model).stats()
        print(f"\nalign stacker: {st}; windows that fit: {sum(fit)} of {len(fit)}")
        # the stacker served exactly the windows that fit; the others, and only they, took today's call directly
        assert st["windows"] == sum(fit) and st["stacked"] + st["solo"] == sum(fit)
        assert len(aligned) == len(fit) - sum(fit) + st["solo"]
    finally:
        TR.release_sessions(model)
        model.close()
