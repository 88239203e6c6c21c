"""Many-stream Silero VAD on the GPU (wlk_vad_group_*, wlk_vad_stream_run_pcm16).  The claim under test is
bit identity: a stream's probabilities and (h, c) are those of its own solo calls whatever is stacked beside it, however
the calls are cut and in whatever order solo and group calls alternate - np.array_equal throughout.  Against the
reference's numbers the grouped path is then held to the solo test's tolerances (test_gpu_vad.py: 2e-5 on the
probabilities, 1e-4 on the state), which bit identity with the solo path implies."""
import functools

import numpy as np
import pytest

from test_vad_host import META, GOLD, WEIGHTS, case_audio
from whisperlivekit_amd import _lib
from whisperlivekit_amd import vad as V

pytestmark = pytest.mark.gpu

NAMES = sorted(META)
audio_of = functools.lru_cache(maxsize=None)(case_audio)


@pytest.fixture(scope="module")
def weights():
    w = V.HipSileroVADWeights(WEIGHTS)
    yield w
    w.close()


def take(cursor, name, n_windows):
    """The next n_windows x 512 samples of a case (cursor: name -> samples consumed)."""
    at = cursor.get(name, 0)
    cursor[name] = at + n_windows * 512
    chunk = audio_of(name)[at:cursor[name]]
    assert len(chunk) == n_windows * 512
    return chunk


def close_all(*objs):
    for o in objs:
        for m in (o if isinstance(o, (list, tuple)) else [o]):
            m.close()


def test_stacked_equals_alone_bitwise(weights):
    names = ["gaps", "speech12", "loud_short_chunks", "noise6", "speech8_ragged"]
    stacked = [V.HipSileroVAD(weights, max_windows=4) for _ in names]       # a group call is not bound by the stream's
    alone = [V.HipSileroVAD(weights, max_windows=64) for _ in names]        # own max_windows: its scratch is the group's
    group = V.HipSileroVADGroup(weights, max_streams=5, max_windows=64)
    cursor = {}
    calls = [((0, 1, 2, 3, 4), (1, 7, 16, 3, 31)),      # one-window entries and the call boundaries carry the context
             ((0, 2, 4), (5, 1, 9)),
             ((4, 3, 2, 1, 0), (2, 1, 13, 8, 1))]       # all five again, other counts, other slots
    for members, counts in calls:
        chunks = [take(cursor, names[i], n) for i, n in zip(members, counts)]
        got = group.probs([stacked[i] for i in members], chunks)
        assert [len(g) for g in got] == list(counts)
        for i, chunk, g in zip(members, chunks, got):
            assert np.array_equal(g, alone[i].probs(chunk)), (members, i)
    for a, b in zip(stacked, alone):
        (ha, ca), (hb, cb) = a.state(), b.state()
        assert np.array_equal(ha, hb) and np.array_equal(ca, cb)
    assert float(max(np.abs(m.state()[0]).max() for m in stacked)) > 0        # not all-zero states compared
    close_all(stacked, alone, group)


def test_grouped_cases_match_the_reference_within_the_solo_tolerances(weights):
    models = [V.HipSileroVAD(weights, max_windows=1) for _ in NAMES]
    group = V.HipSileroVADGroup(weights, max_streams=len(NAMES), max_windows=16 * len(NAMES))
    total = {n: len(audio_of(n)) // 512 for n in NAMES}
    probs, cursor = {n: [] for n in NAMES}, {}
    for lo in range(0, max(total.values()), 16):
        live = [i for i, n in enumerate(NAMES) if total[n] > lo]
        chunks = [take(cursor, NAMES[i], min(16, total[NAMES[i]] - lo)) for i in live]
        for i, p in zip(live, group.probs([models[i] for i in live], chunks)):
            probs[NAMES[i]].append(p)
    for n, m in zip(NAMES, models):
        err = float(np.abs(np.concatenate(probs[n]) - GOLD[n + "_probs"]).max())
        h, c = m.state()
        serr = float(np.abs(np.stack([h, c]) - GOLD[n + "_state"][:, 0, :]).max())
        print(n, "probs err", err, "state err", serr)
        assert err <= 2e-5 and serr <= 1e-4, (n, err, serr)      # test_gpu_vad.py's bounds for the solo path
    close_all(models, group)


def pcm16_of(name, n_windows):
    x = audio_of(name)[: n_windows * 512]
    pcm = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)     # synth.to_pcm16_roundtrip's rounding
    return pcm, pcm.astype(np.float32) / np.float32(32768.0)


def test_int16_input_has_the_bits_of_the_widened_fp32_input(weights):
    (pa, fa), (pb, fb) = pcm16_of("gaps", 40), pcm16_of("loud_short_chunks", 23)
    pb[1000:1004] = (-32768, 32767, -1, 1)                                    # both ends of the range and the smallest steps
    fb = pb.astype(np.float32) / np.float32(32768.0)
    assert np.abs(pa.astype(np.int32)).max() > 3000 and fb.min() == -1.0      # real signal
    f32a, f32b, s16a, g16a, g16b = (V.HipSileroVAD(weights, max_windows=16) for _ in range(5))
    group = V.HipSileroVADGroup(weights, max_streams=2, max_windows=64)
    want_a, want_b = f32a.probs(fa), f32b.probs(fb)
    assert np.array_equal(s16a.probs_pcm16(pa), want_a)                       # 40 windows: three solo calls of <= 16
    got_a, got_b = group.probs([g16a, g16b], [pa, pb])
    assert np.array_equal(got_a, want_a) and np.array_equal(got_b, want_b)
    for m in (s16a, g16a):
        assert all(np.array_equal(u, v) for u, v in zip(m.state(), f32a.state()))
    assert all(np.array_equal(u, v) for u, v in zip(g16b.state(), f32b.state()))
    with pytest.raises(ValueError):
        s16a.probs_pcm16(fa)
    close_all(f32a, f32b, s16a, g16a, g16b, group)


def test_a_stream_alternates_between_solo_and_group_calls(weights):
    mixed, twin, other = (V.HipSileroVAD(weights, max_windows=32) for _ in range(3))
    group = V.HipSileroVADGroup(weights, max_streams=2, max_windows=64)
    cursor, cursor_other = {}, {}
    for k, n in enumerate((3, 16, 1, 9)):
        chunk = take(cursor, "speech12", n)
        if k % 2 == 0:
            got = mixed.probs(chunk)
        else:
            got = group.probs([other, mixed], [take(cursor_other, "gaps", 5), chunk])[1]
        assert np.array_equal(got, twin.probs(chunk)), k
    assert all(np.array_equal(u, v) for u, v in zip(mixed.state(), twin.state()))
    close_all(mixed, twin, other, group)


def test_step_many_reproduces_the_reference_events_for_all_cases_at_once(weights):
    models = [V.HipSileroVAD(weights, max_windows=1) for _ in NAMES]
    its = [V.HipFixedVADIterator(m) for m in models]
    group = V.HipSileroVADGroup(weights, max_streams=len(NAMES), max_windows=256)
    feeds = []
    for n in NAMES:
        audio, chunking, at, k, f = audio_of(n), META[n]["chunking"], 0, 0, []
        while at < len(audio):
            f.append(audio[at:at + chunking[k % len(chunking)]])
            at += chunking[k % len(chunking)]
            k += 1
        feeds.append(f)
    per_call, none = [[] for _ in NAMES], np.zeros(0, np.float32)
    for k in range(max(len(f) for f in feeds)):
        got = V.vad_step_many(group, its, [f[k] if k < len(f) else none for f in feeds])
        for j, ev in enumerate(got):
            if k < len(feeds[j]):
                per_call[j].append(ev)
    for j, n in enumerate(NAMES):
        assert per_call[j] == META[n]["events_per_call"], n
        assert [e for ev in per_call[j] for e in ev] == META[n]["events"], n
    close_all(models, group)


def test_bad_calls_are_refused_and_leave_the_streams_untouched(weights):
    other_weights = V.HipSileroVADWeights(WEIGHTS)
    a, b, c, twin_a, twin_b = (V.HipSileroVAD(weights, max_windows=16) for _ in range(5))
    foreign = V.HipSileroVAD(other_weights, max_windows=16)
    group = V.HipSileroVADGroup(weights, max_streams=2, max_windows=8)
    cursor = {}
    x = audio_of("speech12")
    w = lambda n: x[: n * 512]
    bad_calls = [
        ("duplicate stream", [a, a], [w(1), w(1)]),
        ("zero windows", [a, b], [w(1), w(0)]),
        ("too many streams", [a, b, c], [w(1), w(1), w(1)]),
        ("too many windows", [a, b], [w(4), w(5)]),
        ("stream of other weights", [a, foreign], [w(1), w(1)]),
        ("not a multiple of 512", [a, b], [w(1), x[:700]]),
        ("mixed dtypes", [a, b], [w(1), np.zeros(512, np.int16)]),
    ]
    for what, models, chunks in bad_calls:
        with pytest.raises(_lib.WlkError):
            group.probs(models, chunks)
        # the next valid call continues both streams as if the bad one had not been made
        ca, cb = take(cursor, "gaps", 3), take(cursor, "loud_short_chunks", 2)
        got = group.probs([a, b], [ca, cb])
        assert np.array_equal(got[0], twin_a.probs(ca)) and np.array_equal(got[1], twin_b.probs(cb)), what
    assert all(np.array_equal(u, v) for u, v in zip(a.state() + b.state(), twin_a.state() + twin_b.state()))
    with pytest.raises(_lib.WlkError):
        V.HipSileroVADGroup(weights, max_streams=65)
    with pytest.raises(_lib.WlkError):
        V.HipSileroVADGroup(weights, max_windows=0)
    one = take(cursor, "gaps", 8)                       # a group of one stream, at the group's full capacity
    assert np.array_equal(group.probs([a], [one])[0], twin_a.probs(one))
    close_all(a, b, c, twin_a, twin_b, foreign, group, other_weights)
