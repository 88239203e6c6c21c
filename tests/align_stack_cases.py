"""Shared by tests/test_align_stack_cpu.py and tests/test_gpu_align_group.py: what the device's path walk must return for
a trace, cost matrices with the degenerate contents the walk and the recurrence have to survive, and stand-ins for the
host tests of ``transcribe.AlignStacker``."""
import numpy as np

import helpers as H  # noqa: F401  (puts the repository root on the path)
from oracle import timing_oracle


def starts_of_path(path, n_rows: int) -> np.ndarray:
    """starts[i] = time index of the first path element whose text index is i (i = 0 .. n_rows - 1): what
    ``timing.word_timings`` reads of ``backtrace``'s path (``time_indices[first_of_token]``)."""
    text, time = np.asarray(path[0]), np.asarray(path[1])
    first = np.ones(len(text), dtype=bool)
    first[1:] = text[1:] != text[:-1]
    assert text[first].tolist() == list(range(n_rows)), "the path does not enter every text row once, in order"
    return time[first].astype(np.int32)


def starts_of_trace(trace: np.ndarray) -> np.ndarray:
    return starts_of_path(timing_oracle.backtrace(trace), trace.shape[0] - 1)


def cost_matrix(kind: str, n: int, m: int, seed: int) -> np.ndarray:
    """plain: normal costs; nan_row: one row of NaN; inf_col: one column of +inf; ties: every cost equal (every comparison
    of the recurrence is a tie); quant: costs rounded to a few values (many ties)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, m)).astype(np.float32)
    if kind == "nan_row":
        x[int(rng.integers(n))] = np.nan
    elif kind == "inf_col":
        x[:, int(rng.integers(m))] = np.inf
    elif kind == "ties":
        x[:] = np.float32(0.25)
    elif kind == "quant":
        x = np.round(x)
    elif kind != "plain":
        raise ValueError(kind)
    return x


class WordTokenizer:
    """what timing.find_alignment_many needs of a tokenizer: every text token is a word of its own"""
    sot_sequence = (90,)
    no_timestamps = 91
    eot = 80

    def split_to_word_tokens(self, tokens):
        return [f" w{t}" for t in tokens], [[int(t)] for t in tokens]


class FakeAlignGroup:
    """Stands in for engine.HipWindowGroup: starts and probabilities are a function of the window's own tokens alone, so
    a window's result does not depend on who rode beside it; records the sizes of its calls."""

    def __init__(self, rows: int = 8, refuse=(), break_at=None):
        self.rows, self.refuse, self.break_at = rows, set(refuse), break_at
        self.calls = []

    @staticmethod
    def answer(tokens, n_sot, num_frames):
        text = np.asarray(tokens[n_sot + 1:-1], dtype=np.int64)
        starts = np.minimum(np.arange(len(text) + 1) * 3 + int(text[0]) % 5, num_frames // 2 - 1).astype(np.int32)
        return starts, ((text % 7 + 1) / 8).astype(np.float32)

    def fits(self, n_tokens, num_frames):
        return 9 <= n_tokens <= 256

    def find_alignment(self, windows, want_cost=False, want_trace=False):
        if self.break_at is not None and len(self.calls) == self.break_at:
            self.calls.append(len(windows))
            raise RuntimeError("the device is gone")
        for w in windows:
            if id(w[0]) in self.refuse:
                err = RuntimeError("wlk_hip error -1: refused")
                err.code = -1
                raise err
        self.calls.append(len(windows))
        return [(*self.answer(w[1], w[2], w[4]), None, None) for w in windows]
