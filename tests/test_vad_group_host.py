"""Many-stream Silero VAD, CPU side: the new C ABI is declared and bound, and ``vad_step_many`` drives
each iterator exactly as its own ``__call__`` would - checked with a stand-in group that answers with the probabilities
the REFERENCE computed (tests/golden/vad_cases.npz), so the events must be the reference's (vad_cases.json)."""
import os
import re

import numpy as np
import pytest

from test_vad_host import META, GOLD, case_audio
from whisperlivekit_amd import _lib
from whisperlivekit_amd import vad as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("wlk_vad_stream_run_pcm16", "wlk_vad_group_create", "wlk_vad_group_run", "wlk_vad_group_destroy")
NAMES = sorted(META)


def test_new_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "wlk_hip.h")).read()
    declared = set(re.findall(r"\b(wlk_[a-z_0-9]+)\s*\(", header))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name


class GoldenModel:
    """A stream whose probabilities are the golden ones of ``name``, handed out in order."""

    def __init__(self, name):
        self.name, self.at = name, 0

    def reset_states(self, batch_size=1):
        self.at = 0


class GoldenGroup:
    """Stands in for HipSileroVADGroup: answers each chunk with the next golden probabilities of its model."""

    def __init__(self):
        self.calls = []

    def probs(self, models, chunks):
        assert len(models) == len(chunks) and len(set(map(id, models))) == len(models)
        self.calls.append([m.name for m in models])
        out = []
        for m, c in zip(models, chunks):
            assert c.dtype == np.float32 and len(c) > 0 and len(c) % 512 == 0
            n = len(c) // 512
            out.append(GOLD[m.name + "_probs"][m.at:m.at + n])
            assert len(out[-1]) == n
            m.at += n
        return out


def chunks_of(name):
    audio, chunking, at, k, out = case_audio(name), META[name]["chunking"], 0, 0, []
    while at < len(audio):
        n = chunking[k % len(chunking)]
        out.append(audio[at:at + n])
        at += n
        k += 1
    return out


@pytest.mark.parametrize("name", NAMES)
def test_step_many_emits_the_reference_events_beside_other_streams(name):
    i = NAMES.index(name)
    names = [name, NAMES[(i + 1) % len(NAMES)], NAMES[(i + 2) % len(NAMES)]]
    feeds = [chunks_of(n) for n in names]
    its = [V.HipFixedVADIterator(GoldenModel(n)) for n in names]
    group, none = GoldenGroup(), np.zeros(0, np.float32)
    per_call = [[] for _ in names]
    for k in range(len(feeds[0])):                       # a companion that runs out of audio gets empty chunks
        got = V.vad_step_many(group, its, [f[k] if k < len(f) else none for f in feeds])
        for j, ev in enumerate(got):
            if k < len(feeds[j]):
                per_call[j].append(ev)
    assert per_call[0] == META[name]["events_per_call"]
    assert [e for ev in per_call[0] for e in ev] == META[name]["events"]
    for j in (1, 2):                                     # the companions too, as far as they were fed
        assert per_call[j] == META[names[j]]["events_per_call"][:len(per_call[j])]
    assert any(len(c) == 3 for c in group.calls)         # the three really shared calls


def test_step_many_skips_an_iterator_without_a_complete_window():
    a, b = V.HipFixedVADIterator(GoldenModel("gaps")), V.HipFixedVADIterator(GoldenModel("speech12"))
    group = GoldenGroup()
    x = case_audio("gaps")
    got = V.vad_step_many(group, [a, b], [x[:300], case_audio("speech12")[:1024]])
    assert got[0] == [] and group.calls == [["speech12"]]
    assert np.array_equal(a.buffer, x[:300]) and len(b.buffer) == 0 and a.current_sample == 0 and b.current_sample == 1024
    got = V.vad_step_many(group, [a, b], [x[300:600], np.zeros(100, np.float32)])
    assert group.calls[-1] == ["gaps"] and np.array_equal(a.buffer, x[512:600]) and len(b.buffer) == 100
    assert got[0] == META["gaps"]["events_per_call"][0] and got[1] == []      # window 0 of "gaps" opens its first segment
    assert V.vad_step_many(group, [a, b], [np.zeros(0, np.float32)] * 2) == [[], []] and len(group.calls) == 2
    with pytest.raises(ValueError):
        V.vad_step_many(group, [a, b], [x[:512]])
