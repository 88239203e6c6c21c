"""The host half of the stacked word alignment: ``timing.word_timings_from_starts`` against the path-based
``word_timings``, ``transcribe.AlignStacker`` over a stand-in group, the switches, and the ABI lists."""
import os
import re
import threading

import numpy as np
import pytest

import helpers as H
import align_stack_cases as AC
from oracle import timing_oracle
from whisperlivekit_amd import _lib, timing, transcribe as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = H.golden_json("word_timing_kat.json")
NEW_SYMBOLS = ("wlk_group_find_alignment", "wlk_group_align_fits", "wlk_diag_dtw_starts")


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g.word, g.tokens) == (w.word, w.tokens)
        assert g.start == w.start and g.end == w.end and g.probability == w.probability


# ---- 1. word_timings_from_starts -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", KAT["find_alignment"], ids=lambda c: c["text"].strip()[:12])
def test_from_starts_equals_from_the_path_on_the_reference_matrices(case):
    x = np.array(case["matrix"], dtype=np.float32).reshape(case["matrix_shape"])
    trace = timing_oracle.dtw_trace(x)
    path = timing.backtrace(trace)
    np.testing.assert_array_equal(path, np.array(case["path"]))
    starts = AC.starts_of_trace(trace)
    assert len(starts) == len(case["text_tokens"]) + 1
    want = timing.word_timings(*path, case["words"], case["word_tokens"], case["text_token_probs"])
    assert len(want) == len(case["timings"])
    _same(timing.word_timings_from_starts(starts, case["words"], case["word_tokens"], case["text_token_probs"]), want)


@pytest.mark.parametrize("seed", range(50))
def test_from_starts_equals_from_the_path_on_random_traces(seed):
    rng = np.random.default_rng(1000 + seed)
    kind = ("plain", "nan_row", "inf_col", "quant", "ties")[seed % 5]
    n, m = int(rng.integers(2, 41)), int(rng.integers(1, 61))
    trace = timing_oracle.dtw_trace(AC.cost_matrix(kind, n, m, seed))
    path = timing.backtrace(trace)
    # words of 1..3 tokens over the n - 1 text tokens, the eot pseudo-word behind them
    sizes = []
    while sum(sizes) < n - 1:
        sizes.append(min(int(rng.integers(1, 4)), n - 1 - sum(sizes)))
    ids = iter(range(n - 1))
    word_tokens = [[next(ids) for _ in range(k)] for k in sizes] + [[999]]
    words = [f" w{i}" for i in range(len(word_tokens))]
    probs = rng.random(n - 1).astype(np.float32).tolist()
    want = timing.word_timings(*path, words, word_tokens, probs)
    _same(timing.word_timings_from_starts(AC.starts_of_trace(trace), words, word_tokens, probs), want)
    assert timing.word_timings_from_starts([0], ["<eot>"], [[999]], []) == []


# ---- 2. AlignStacker over a stand-in group ----------------------------------------------------------------------------------------
class Sess:
    pass


def _want(tokens_of_text, num_frames):
    tok = AC.WordTokenizer()
    tokens, n_sot = timing.alignment_tokens(tok, tokens_of_text)
    starts, probs = AC.FakeAlignGroup.answer(tokens, n_sot, num_frames)
    words, word_tokens = tok.split_to_word_tokens(list(tokens_of_text) + [tok.eot])
    return timing.word_timings_from_starts(starts, words, word_tokens, probs.tolist())


class GatedGroup(AC.FakeAlignGroup):
    """lets a test hold the runner inside a pass while other threads queue their windows"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.entered, self.go = threading.Event(), threading.Event()

    def find_alignment(self, windows, **k):
        if not self.calls:
            self.entered.set()
            assert self.go.wait(60)
        return super().find_alignment(windows, **k)


def _threads(stacker, jobs):
    out, errors = [None] * len(jobs), [None] * len(jobs)

    def work(i):
        try:
            out[i] = stacker.align(*jobs[i])
        except BaseException as e:
            errors[i] = e
    return [threading.Thread(target=work, args=(i,)) for i in range(len(jobs))], out, errors


def _join_all(ts):
    for t in ts:
        t.join(60)
    assert not any(t.is_alive() for t in ts), "a waiter is still blocked"


def _wait_queued(stacker, n):
    while True:
        with stacker._cv:
            if len(stacker._queue) == n:
                return


TEXTS = [[3, 4, 5, 6, 7, 8, 9], [11, 12, 13, 14, 15, 16], [21, 22, 23, 24, 25, 26, 27, 28]]


def _jobs():
    return [(Sess(), AC.WordTokenizer(), text, 1000 + 100 * i) for i, text in enumerate(TEXTS)]


def test_windows_queued_during_a_pass_ride_the_next_one():
    group = GatedGroup(8)
    stacker = TR.AlignStacker(None, 8, group=group)
    jobs = _jobs()
    ts, out, errors = _threads(stacker, jobs)
    ts[0].start()
    assert group.entered.wait(60)                      # the first caller drives and sits in its pass of one
    ts[1].start(); ts[2].start()
    _wait_queued(stacker, 2)
    group.go.set()
    _join_all(ts)
    assert errors == [None] * 3 and group.calls == [1, 2]
    for got, (_s, _t, text, frames) in zip(out, jobs):
        _same(got, _want(text, frames))
    st = stacker.stats()
    assert (st["passes"], st["windows"], st["group_passes"], st["stacked"], st["solo"]) == (1, 3, 2, 3, 0)
    assert not stacker._running and not stacker._open and not stacker._queue


def test_more_windows_than_rows_take_several_passes():
    group = AC.FakeAlignGroup(2)
    stacker = TR.AlignStacker(None, 2, group=group)
    windows = [TR._AlignWindow(*job) for job in _jobs()]
    stacker.run_many(windows)
    assert group.calls == [2, 1]
    for w, (_s, _t, text, frames) in zip(windows, _jobs()):
        _same(w.result, _want(text, frames))


def test_a_refused_window_is_aligned_solo_and_the_others_are_unaffected(monkeypatch):
    jobs = _jobs()
    group = AC.FakeAlignGroup(8, refuse=[id(jobs[1][0])])
    solo_calls = []

    def solo(session, tokenizer, text_tokens, mel, num_frames):
        solo_calls.append((session, mel, num_frames))
        return ["solo", list(text_tokens)]
    monkeypatch.setattr(TR.T, "find_alignment", solo)
    stacker = TR.AlignStacker(None, 8, group=group)
    windows = [TR._AlignWindow(*job) for job in jobs]
    stacker.run_many(windows)
    # the pass of three was refused as a whole (nobody touched), then every window on its own: two pass, one goes solo
    assert group.calls == [1, 1] and solo_calls == [(jobs[1][0], None, jobs[1][3])]
    _same(windows[0].result, _want(TEXTS[0], jobs[0][3]))
    assert windows[1].result == ["solo", TEXTS[1]]
    _same(windows[2].result, _want(TEXTS[2], jobs[2][3]))
    assert stacker.stats()["solo"] == 1 and stacker.stats()["windows"] == 3

    def broken(*a):
        raise ValueError("its own error")
    monkeypatch.setattr(TR.T, "find_alignment", broken)
    with pytest.raises(ValueError, match="its own error"):      # what stops a window on its own chain is its own error
        stacker.align(*jobs[1])
    _same(stacker.align(*jobs[0]), _want(TEXTS[0], jobs[0][3]))


def test_a_failing_pass_wakes_every_waiter_with_the_error():
    group = GatedGroup(8, break_at=1)
    stacker = TR.AlignStacker(None, 8, group=group)
    jobs = _jobs() + [(Sess(), AC.WordTokenizer(), [31, 32, 33, 34, 35, 36], 900)]
    ts, out, errors = _threads(stacker, jobs)
    ts[0].start()
    assert group.entered.wait(60)
    ts[1].start(); ts[2].start()
    _wait_queued(stacker, 2)
    group.go.set()                                     # call 0 (one window) goes through, call 1 (two windows) dies
    _join_all(ts[:3])
    assert errors[0] is None and out[0] is not None
    assert all(isinstance(e, RuntimeError) and "device is gone" in str(e) for e in errors[1:3]), errors
    assert not stacker._running and not stacker._open and not stacker._queue
    ts[3].start()                                      # the next caller drives a fresh pass
    _join_all(ts[3:])
    assert errors[3] is None
    _same(out[3], _want(jobs[3][2], 900))


def test_a_lone_window_goes_solo_only_when_asked(monkeypatch):
    monkeypatch.setattr(TR.T, "find_alignment", lambda *a: "solo")
    job = _jobs()[0]
    group = AC.FakeAlignGroup(8)
    assert TR.AlignStacker(None, 8, group=group, solo_single=True).align(*job) == "solo" and group.calls == []
    _same(TR.AlignStacker(None, 8, group=group, solo_single=False).align(*job), _want(job[2], job[3]))
    assert group.calls == [1]
    with pytest.raises(ValueError):
        TR.AlignStacker(None, 9, group=group)


# ---- the switches ---------------------------------------------------------------------------------------------------------------
class Model:
    pass


class FakeWindows:
    def __init__(self, model, rows):
        self.rows, self.group = rows, AC.FakeAlignGroup(rows)


def test_switch_off_constructs_nothing_and_the_argument_wins(monkeypatch):
    monkeypatch.delenv("WLK_TRANSCRIBE_ALIGN_STACK", raising=False)
    monkeypatch.setenv("WLK_TRANSCRIBE_STACK", "4")
    monkeypatch.setattr(TR, "WindowStacker", FakeWindows)
    real = TR.AlignStacker

    def never(*a, **k):
        raise AssertionError("constructed although the switch is off")
    monkeypatch.setattr(TR, "AlignStacker", never)
    m = Model()
    assert TR.resolve_align_stack(None) is False and TR._align_stacker(m) is None and TR.align_stacker(m) is None
    assert "_align_stacker" not in m.__dict__ and "_window_stacker" not in m.__dict__
    monkeypatch.setenv("WLK_TRANSCRIBE_ALIGN_STACK", "1")
    assert TR.resolve_align_stack(None) is True
    assert TR.set_align_stack(m, False) is False and TR._align_stacker(m) is None       # the argument wins
    monkeypatch.setenv("WLK_TRANSCRIBE_STACK", "0")
    assert TR.set_align_stack(m, True) is True and TR._align_stacker(m) is None         # needs the stacked windows
    assert "_window_stacker" not in m.__dict__
    monkeypatch.setattr(TR, "AlignStacker", real)
    monkeypatch.setenv("WLK_TRANSCRIBE_STACK", "4")
    st = TR._align_stacker(m)
    assert isinstance(st, real) and st.rows == 4 and st.group is TR.window_stacker(m).group      # the one group of the model
    assert TR._align_stacker(m) is st and TR.align_stacker(m) is st
    monkeypatch.delenv("WLK_TRANSCRIBE_ALIGN_STACK")
    assert TR.set_align_stack(m, None) is False and TR._align_stacker(m) is None


def test_routing_of_a_windows_alignment(monkeypatch):
    """Stacked only when the switch is on, the 1-row session holds the window and the shape fits; today's call otherwise."""
    monkeypatch.setenv("WLK_TRANSCRIBE_STACK", "4")
    monkeypatch.setenv("WLK_TRANSCRIBE_ALIGN_STACK", "1")
    monkeypatch.setattr(TR, "WindowStacker", FakeWindows)
    solo = []
    monkeypatch.setattr(TR.T, "find_alignment", lambda s, t, text, mel, nf: solo.append((s, mel)) or "solo")
    seen = []
    monkeypatch.setattr(TR.T, "attach_words", lambda segments, alignment, per_segment, **k: seen.append(alignment))
    rows = Sess()
    monkeypatch.setattr(TR, "_rows_of", lambda model: {1: rows})
    m, tok, sess = Model(), AC.WordTokenizer(), Sess()
    seg = lambda n: [dict(tokens=list(range(1, n + 1)) + [tok.eot + 5], seek=0)]          # noqa: E731
    args = (m, tok, "mel", 3000, "", "", 0.0)
    TR._add_word_timestamps(seg(7), sess, *args)                   # 1 + 2 + 7 = 10 tokens: fits
    _same(seen[-1], _want(list(range(1, 8)), 3000))
    assert solo == [] and TR.align_stacker(m).stats()["stacked"] == 1
    TR._add_word_timestamps(seg(5), sess, *args)                   # 8 tokens: below the stacked range
    assert seen[-1] == "solo" and solo == [(sess, None)]
    TR._add_word_timestamps(seg(7), None, *args)                   # decoded in a several-row session: re-encode branch
    assert seen[-1] == "solo" and solo[-1] == (rows, "mel")
    TR.set_align_stack(m, False)
    TR._add_word_timestamps(seg(7), sess, *args)
    assert seen[-1] == "solo" and len(solo) == 3 and TR.align_stacker(m).stats()["windows"] == 1


def test_asr_wrapper_switch(monkeypatch):
    from whisperlivekit_amd.local_agreement import HipWhisperASR
    monkeypatch.delenv("WLK_TRANSCRIBE_STACK", raising=False)
    monkeypatch.delenv("WLK_TRANSCRIBE_ALIGN_STACK", raising=False)
    m = Model()
    asr = HipWhisperASR("en", hip_model=m)
    assert asr.align_stack is False and "_align_stack" not in m.__dict__
    assert HipWhisperASR("en", hip_model=m, stack=3, align_stack=True).align_stack is True and m.__dict__["_align_stack"] is True
    with pytest.raises(ValueError):
        HipWhisperASR("en", hip_model=Model(), stack=0, align_stack=True)
    monkeypatch.setenv("WLK_TRANSCRIBE_ALIGN_STACK", "1")
    assert HipWhisperASR("en", hip_model=Model(), stack=2).align_stack is True
    assert HipWhisperASR("en", hip_model=Model(), stack=2, align_stack=False).align_stack is False
    assert HipWhisperASR("en", hip_model=Model()).align_stack is False               # needs stack >= 1


# ---- 3. ABI ------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_listed_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "wlk_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in include/wlk_hip.h"
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name).argtypes, name
    assert "wlk_group_find_alignment" in integration and "WLK_TRANSCRIBE_ALIGN_STACK" in integration
    fields = re.search(r"typedef struct wlk_align_window \{(.*?)\} wlk_align_window;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n.strip(" *") for decl in fields.split(";") if decl.strip() for n in decl.split(",")]
    names = [n.split()[-1].strip("*") for n in names]
    assert names == [n for n, _t in _lib.AlignWindow._fields_]


def test_refusals_need_no_device():
    lib = _lib.load()
    fits = _lib.C.c_int32(7)
    assert lib.wlk_group_align_fits(None, 10, 3000, _lib.C.byref(fits)) == -1
    assert lib.wlk_group_find_alignment(None, None, 1) == -1
    one = np.zeros(4, np.float32)
    off, nr, nc = np.zeros(1, np.int64), np.ones(1, np.int32), np.ones(1, np.int32)
    starts = np.full(4, -77, np.int32)
    vp = lambda a: a.ctypes.data_as(_lib.C.c_void_p)               # noqa: E731
    for n, rows, cols in ((0, 1, 1), (9, 1, 1), (1, 0, 1), (1, 1025, 1), (1, 1, 0), (1, 1, 4096)):
        nr[0], nc[0] = rows, cols
        assert lib.wlk_diag_dtw_starts(vp(one), vp(off), vp(nr), vp(nc), n, vp(starts), None) == -1, (n, rows, cols)
    assert lib.wlk_diag_dtw_starts(None, vp(off), vp(nr), vp(nc), 1, vp(starts), None) == -1
    assert (starts == -77).all()
