"""LocalAgreement's batch Whisper on the HIP library: ``transcribe()`` = the 30-second window loop with
temperature fallback of ``whisperlivekit/whisper/transcribe.py:21-494``, ``decode()`` = one window through the
``DecodingTask`` of ``whisperlivekit/whisper/decoding.py:502-784`` (prompt / prefix assembly, blank / annotation / timestamp
rules, greedy, sampling and beam search, ranking), ``detect_language()`` = ``decoding.py:19-77``.

What runs where: the log-mel of the whole recording (``wlk_log_mel``), the encoder and cross-K/V of each window
(``wlk_encode_mel``), every decoder step with its KV cache (``wlk_decode`` / ``wlk_kv_reorder``), the no-speech probability
and the device half of the word alignment (``wlk_find_alignment``) are HIP kernels.  The per-step logit rules are a handful
of masked fills and one log-softmax over the vocabulary row the step produced; they run on that row on the host
(single-threaded numpy; the sampling draw takes its random numbers from torch's global generator exactly as the reference's
``Categorical.sample()`` does, so a seeded run consumes the generator as the reference does); greedy decoding at temperature 0
applies them on the device (``wlk_pick_greedy``), and so does beam search with 2-7 beams under WLK_TRANSCRIBE_DEVICE_BEAM=1
(``wlk_pick_topk``, with single-token steps over the KV ancestry table: ``wlk_decode_ancestry``).  With WLK_TRANSCRIBE_STACK=n
(or ``HipWhisperASR(stack=n)``; off by default) the greedy temperature-0 steps of up to n concurrent windows of one model
ride in one launch chain per token (``WindowStacker`` / ``decode_many`` over ``wlk_group_step_pick``); with
WLK_TRANSCRIBE_ALIGN_STACK=1 on top of it (or ``HipWhisperASR(stack=n, align_stack=True)``; off by default) the word alignment of
the windows those calls have waiting shares one stacked pass as well (``AlignStacker`` over ``wlk_group_find_alignment``).
With a ``draft`` (``DecodingOptions.draft``, ``decode_many(drafts=...)``, ``transcribe(draft=WindowDraft)``; off unless given) a
stacked greedy window opens with ONE teacher-forced pass that verifies the tokens an earlier call sampled
(``wlk_group_verify``) instead of a prefill and one step per token already known.
There is no CPU model path: without the library / a GPU the first call raises.

Same keyword names, defaults and result dictionary as the reference; ``fp16`` is accepted and ignored (the path computes
in fp32, as the reference does on its CPU).  Decoding a file name (ffmpeg) is outside the path: ``audio`` is samples.
"""
from __future__ import annotations

import os
import threading
import warnings
import zlib
from dataclasses import dataclass, field, replace
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import timing as T
from .engine import HipSession, HipWhisperModel
from .policy import BeamUpdate
from .tokenizer import WhisperTokenizer, get_tokenizer

SAMPLE_RATE, HOP_LENGTH, CHUNK_LENGTH = 16000, 160, 30
N_SAMPLES = CHUNK_LENGTH * SAMPLE_RATE          # 480000
N_FRAMES = N_SAMPLES // HOP_LENGTH              # 3000
FRAMES_PER_SECOND = SAMPLE_RATE // HOP_LENGTH   # 100
NEG_INF = float("-inf")


# ---- options / result (decoding.py:80-127) ----------------------------------------------------------------------------------
@dataclass(frozen=True)
class DecodingOptions:
    task: str = "transcribe"
    language: Optional[str] = None
    temperature: float = 0.0
    sample_len: Optional[int] = None
    best_of: Optional[int] = None
    beam_size: Optional[int] = None
    patience: Optional[float] = None
    length_penalty: Optional[float] = None
    prompt: Optional[Union[str, List[int]]] = None
    prefix: Optional[Union[str, List[int]]] = None
    suppress_tokens: Optional[Union[str, Iterable[int]]] = "-1"
    suppress_blank: bool = True
    without_timestamps: bool = False
    max_initial_timestamp: Optional[float] = 1.0
    fp16: bool = False            # accepted for signature compatibility; the HIP path is fp32
    # not in the reference: the tokens an earlier decode of (a prefix of) this window sampled; the greedy temperature-0
    # path verifies them in one decoder pass instead of re-deriving them token by token
    draft: Optional[Sequence[int]] = None


@dataclass(frozen=True)
class DecodingResult:
    audio_features: object = None             # stays on the device (the session's cross-K/V); kept for field parity
    language: str = "en"
    language_probs: Optional[Dict[str, float]] = None
    tokens: List[int] = field(default_factory=list)
    text: str = ""
    avg_logprob: float = float("nan")
    no_speech_prob: float = float("nan")
    temperature: float = float("nan")
    compression_ratio: float = float("nan")


def compression_ratio(text: str) -> float:
    """utils.py:45-47."""
    raw = text.encode("utf-8")
    return len(raw) / len(zlib.compress(raw))


def pad_or_trim(mel: np.ndarray, length: int = N_FRAMES) -> np.ndarray:
    """audio.py:65-88 on the last axis: cut, or fill with ZEROS (not with the mel's silence value)."""
    if mel.shape[-1] > length:
        mel = mel[..., :length]
    if mel.shape[-1] < length:
        mel = np.pad(mel, [(0, 0)] * (mel.ndim - 1) + [(0, length - mel.shape[-1])])
    return np.ascontiguousarray(mel, dtype=np.float32)


def choose(logits: torch.Tensor, temperature: float) -> torch.Tensor:
    """GreedyDecoder's choice (decoding.py:274-277) on the filtered logits [rows, vocabulary]: arg-max at temperature 0,
    else one categorical draw per row from torch's global generator.  Module-level so that the parity tests can follow
    the reference's recorded choices step by step."""
    if temperature == 0:
        return torch.from_numpy(logits.numpy().argmax(axis=-1))
    return _categorical_draw(logits.numpy() / np.float32(temperature))


def _categorical_draw(scaled: np.ndarray) -> torch.Tensor:
    """``Categorical(logits=scaled).sample()`` with the same consumption of torch's global generator and the same result:
    a single draw per row goes through ``torch.multinomial``'s one-sample path, argmax(p / q) with q ~ Exp(1) drawn per
    vocabulary entry.  Only the exponentials come from torch (that is the generator's part); the softmax, the division and
    the arg-max are single-threaded numpy - torch hands each of these 50k-element rows to its whole intra-op pool (34 ms
    per draw on a 128-thread host).  tests/test_transcribe.py::test_categorical_draw_is_torchs pins the equivalence."""
    m = scaled.max(axis=-1, keepdims=True)
    e = np.exp(scaled - m)
    p = e / e.sum(axis=-1, keepdims=True, dtype=np.float32)
    q = torch.empty(p.shape, dtype=torch.float32).exponential_(1)
    return torch.from_numpy((p / q.numpy()).argmax(axis=-1))


# ---- the model-side handle --------------------------------------------------------------------------------------------------
class _Rows:
    """Sessions of one HipWhisperModel for the batch path, by row count (greedy / sampling: 1 row; best_of / beam: n).
    One set per calling thread: the reference's `transcribe` is re-entrant on a shared model (LocalAgreement serves every
    connection from one WhisperASR, audio_processor.py runs them in worker threads), so concurrent calls must not share
    device state."""

    def __init__(self, model: HipWhisperModel):
        self.model = model
        self.sessions: Dict[int, HipSession] = {}

    def get(self, rows: int) -> HipSession:
        s = self.sessions.get(rows)
        if s is None:
            # its own stream, no batch engine: the audio ring is not used (windows arrive as mel segments)
            s = self.sessions[rows] = self.model.new_session(beam=rows, max_audio_seconds=1.0, batched=False)
        return s

    def windows(self, n: int) -> List[HipSession]:
        """n one-row sessions for the windows of one `decode_many`: the thread's one-row session first, the further ones
        under the keys -1, -2, ... (one-row sessions as well; released with the rest)."""
        out = [self.get(1)]
        for i in range(1, n):
            s = self.sessions.get(-i)
            if s is None:
                s = self.sessions[-i] = self.model.new_session(beam=1, max_audio_seconds=1.0, batched=False)
            out.append(s)
        return out


_ROWS_LOCK = threading.Lock()


def _rows_of(model: HipWhisperModel) -> _Rows:
    key = threading.get_ident()
    stale = []
    with _ROWS_LOCK:
        per_thread = model.__dict__.setdefault("_batch_rows", {})
        r = per_thread.get(key)
        if r is None:
            alive = {t.ident for t in threading.enumerate()}
            stale = [per_thread.pop(k) for k in list(per_thread) if k not in alive]     # threads that have ended
            r = per_thread[key] = _Rows(model)
    for rows in stale:
        for sess in rows.sessions.values():
            sess.close()
    return r


def release_sessions(model: HipWhisperModel) -> None:
    """Close the batch-path sessions every thread created on `model` (call before closing the model)."""
    with _ROWS_LOCK:
        per_thread = model.__dict__.pop("_batch_rows", {})
    for rows in per_thread.values():
        for sess in rows.sessions.values():
            sess.close()


# ---- stacked greedy windows (opt-in; csrc/window_group.hip) -----------------------------------------------------------------
def resolve_stack(stack: Optional[int]) -> int:
    """``HipWhisperASR(stack=...)`` / :func:`set_stack`: an explicit value wins; ``None`` reads ``WLK_TRANSCRIBE_STACK``
    (default 0 = off; 1..8 = rows of the window group)."""
    if stack is None:
        stack = int(os.environ.get("WLK_TRANSCRIBE_STACK", "0").strip() or 0)
    stack = int(stack)
    if stack < 0 or stack > 8:
        raise ValueError("stack must be 0 (off) or 1..8 rows")
    return stack


def resolve_burst(burst: Optional[int]) -> int:
    """``HipWhisperASR(burst=...)`` / :func:`set_burst` / ``WindowStacker(burst=...)``: an explicit value wins; ``None`` reads
    ``WLK_TRANSCRIBE_STACK_BURST`` (default 1 = one step per library call; 2..16 = steps of a window group per call)."""
    if burst is None:
        burst = int(os.environ.get("WLK_TRANSCRIBE_STACK_BURST", "1").strip() or 1)
    burst = int(burst)
    if burst < 1 or burst > 16:
        raise ValueError("burst must be 1..16 steps per call")
    return burst


def _next_pick_state(state: dict, token: int) -> dict:
    """The rule state of the step after ``token`` was picked under ``state``: `_pick_state(history + [token])` as a function
    of `_pick_state(history)` and the pick alone - the host statement of what ``wlk_group_run_pick`` advances on the device
    (csrc/common.h: pick_rules_advance).  The last timestamp of the history is recovered from the old state: ``ts_bound``
    itself when the last token opened a pair (``ts_mode`` 2), ``ts_bound - 1`` when there is a bound at all, none otherwise."""
    tb = state["timestamp_begin"]
    last_ts = token >= tb
    before_last_ts = True if state["first_step"] else state["ts_mode"] != 0
    stamp = None
    if state["ts_mode"] == 2:
        stamp = state["ts_bound"]
    elif state["ts_bound"] > tb:
        stamp = state["ts_bound"] - 1
    if last_ts:
        stamp = int(token)
    mode = 0 if not last_ts else (1 if before_last_ts else 2)
    bound = tb if stamp is None else (stamp if mode == 2 else stamp + 1)
    return dict(state, first_step=False, ts_mode=mode, ts_bound=bound)


def _greedy_take(tokens: np.ndarray, sum_logprobs: np.ndarray, nxt_id: int, picked: float, eot: int,
                 n_ctx: int) -> Tuple[np.ndarray, bool]:
    """GreedyDecoder.update (decoding.py:270-287) for the one sequence of a greedy window whose rules and pick ran on the
    device: the log-probability counts unless the sequence had ended, the token is appended.  -> (tokens, the window is
    over).  The one statement of it for the solo loop and the stacked one."""
    if tokens[0, -1] != eot:
        sum_logprobs[0] += np.float32(picked)
    else:
        nxt_id = eot
    tokens = np.concatenate([tokens, np.asarray([[nxt_id]], np.int64)], axis=1)
    return tokens, bool(nxt_id == eot or tokens.shape[-1] > n_ctx)


def _accept_draft(picks: Sequence[Tuple[int, float]], draft: Sequence[int], eot: Optional[int] = None,
                  ended: bool = False) -> Tuple[int, int, np.float32, np.float32]:
    """How far the greedy loop follows ``draft``: the host statement of ``draft_accept_kernel`` (csrc/select.hip).
    ``picks[j]`` = (token, log-probability) of the greedy pick behind ``draft[:j]``, j = 0 .. len(draft).  -> (k, next
    token, its log-probability, sum): k = the first position whose pick is not the draft's token (len(draft) when there
    is none), next = the pick at k, sum = the log-probabilities of positions 0 .. k added in that order in float32 - the
    order in which `_greedy_take` accumulates.  ``ended``: the token in front of position 0 is ``eot`` already; as in
    `_greedy_take` the sequence then takes ``eot`` whatever was picked and nothing is added."""
    n = len(draft)
    if len(picks) != n + 1:
        raise ValueError("one pick per draft position and one behind the draft")
    k = n
    for j in range(n):
        if int(picks[j][0]) != int(draft[j]) or (ended and j == 0):
            k = j
            break
    total = np.float32(0.0)
    for j in range(1 if ended else 0, k + 1):
        total = np.float32(total + np.float32(picks[j][1]))
    nxt = int(eot) if (ended and k == 0) else int(picks[k][0])
    return k, nxt, np.float32(picks[k][1]), total


def clamp_draft(draft: Optional[Sequence[int]], n_initial: int, sample_len: int, n_ctx: int, eot: int) -> List[int]:
    """The part of ``draft`` a verify pass may carry behind ``n_initial`` initial tokens: cut in front of its first
    <|endoftext|> (a sampled history never holds one), then to min(sample_len - 1, n_ctx - n_initial - 1, 256 - n_initial)
    tokens - the window samples at most ``sample_len`` tokens and the pick behind the draft is one of them, that pick's
    token still needs a text position, and the stacked pass takes 256 rows."""
    out = []
    for t in draft or []:
        if int(t) == eot:
            break
        out.append(int(t))
    room = min(sample_len - 1, n_ctx - n_initial - 1, 256 - n_initial)
    return out[:max(room, 0)]


class WindowDraft:
    """What one LocalAgreement session remembers between two ``transcribe`` calls on its growing buffer: the tokens the
    first window of the last call sampled, and the audio that call saw.  :meth:`begin` hands the tokens out as the next
    call's draft when the new audio begins with the remembered audio sample for sample; a buffer that was trimmed (or any
    other audio) gets none.  Not shared between sessions and not thread-safe: one per session."""

    def __init__(self):
        self.tokens: List[int] = []
        self.audio: Optional[np.ndarray] = None
        self.offered = 0               # calls that were handed a draft
        self.dropped = 0               # calls whose audio did not extend the remembered audio

    def begin(self, audio: np.ndarray) -> List[int]:
        """-> the draft for a call over ``audio`` (may be empty); the memory now holds ``audio`` and no tokens."""
        audio = np.asarray(audio, dtype=np.float32).reshape(-1)
        prev, tokens = self.audio, self.tokens
        self.audio, self.tokens = audio.copy(), []
        if prev is None or not tokens:
            return []
        n = min(len(prev), len(audio))
        if n == 0 or not np.array_equal(prev[:n], audio[:n]):
            self.dropped += 1
            return []
        self.offered += 1
        return list(tokens)

    def remember(self, tokens: Sequence[int]) -> None:
        self.tokens = [int(t) for t in tokens]

    def reset(self) -> None:
        self.tokens, self.audio = [], None


class _GreedyWindow:
    """One greedy temperature-0 window between its first pick and its end, as the stacked loop advances it: the session
    that holds its caches, its tokens and log-probability sum, the steps it may still take."""

    def __init__(self, decoder: "_WindowDecoder", session, tokens: np.ndarray, sum_logprobs: np.ndarray, steps_left: int):
        self.decoder, self.session = decoder, session
        self.tokens, self.sum_logprobs, self.steps_left = tokens, sum_logprobs, int(steps_left)

    def feed(self) -> int:
        return int(self.tokens[0, -1])

    def state(self) -> dict:
        return self.decoder._pick_state(self.tokens)

    def take(self, nxt_id: int, picked: float) -> bool:
        """-> the window is over (<|endoftext|>, sample_len or n_ctx)"""
        self.tokens, over = _greedy_take(self.tokens, self.sum_logprobs, int(nxt_id), float(picked), self.decoder.tok.eot,
                                         self.decoder.n_ctx)
        self.steps_left -= 1
        return over or self.steps_left <= 0


def _refused(error: BaseException) -> bool:
    """the group refused the call on the host (WLK_ERR_ARG / WLK_ERR_STATE): nothing was launched, no session advanced"""
    return getattr(error, "code", None) in (-1, -3)


class _StackerFront:
    """The thread-safe queue in front of one ``HipWindowGroup``, modelled on ``translation.NllbStacker`` and shared by
    :class:`WindowStacker` and :class:`AlignStacker`: any thread hands its items to :meth:`run_many`; the first caller
    becomes the runner and calls ``_advance`` on everything in flight until nothing is in flight or queued, callers that
    arrive while a pass is running queue their items - the runner admits them before its next ``_advance``, up to the
    group's rows - and wait on a condition.  ``_advance(live) -> still live`` settles each item that is over (or failed
    alone) with :meth:`_settle`.  A pass that raises hands its error to every item in flight or queued, so no waiter
    blocks for ever, and the next caller starts a fresh pass."""

    def __init__(self, rows: int):
        if not 1 <= int(rows) <= 8:
            raise ValueError("a window stacker has 1..8 rows")
        self.rows = int(rows)
        self._cv = threading.Condition()
        self._queue: List[Tuple[int, object]] = []            # (ticket, item) not yet admitted
        self._open: set = set()                               # tickets queued or in flight
        self._outcome: dict = {}                              # ticket -> error or None
        self._running = False
        self._next_ticket = 0
        self.passes = 0
        self.windows = 0

    def _advance(self, live: list) -> list:
        raise NotImplementedError

    def run_many(self, windows: Sequence) -> None:
        if not windows:
            return
        with self._cv:
            tickets = list(range(self._next_ticket, self._next_ticket + len(windows)))
            self._next_ticket += len(windows)
            for t, w in zip(tickets, windows):
                self._queue.append((t, w))
                self._open.add(t)
        while True:
            with self._cv:
                while self._running and any(t not in self._outcome for t in tickets):
                    self._cv.wait()
                if all(t in self._outcome for t in tickets):
                    for err in [self._outcome.pop(t) for t in tickets]:
                        if err is not None:
                            raise err
                    return
                self._running = True               # nobody is driving the group and this caller still waits: it drives
            self._run()

    def _settle(self, ticket: int, error: Optional[BaseException]) -> None:
        with self._cv:
            self._outcome[ticket] = error
            self._open.discard(ticket)
            self.windows += 1
            self._cv.notify_all()

    def _run(self) -> None:
        error: Optional[BaseException] = None
        live: list = []
        try:
            while True:
                with self._cv:
                    while self._queue and len(live) < self.rows:
                        live.append(self._queue.pop(0))
                if not live:
                    break
                live = self._advance(live)
        except BaseException as e:                 # the pass is gone: everyone in it or queued behind it gets the error
            error = e
        finally:
            with self._cv:
                self.passes += 1
                if error is not None:
                    for t in self._open:
                        self._outcome[t] = error
                    self._open.clear()
                    self._queue = []
                self._running = False
                self._cv.notify_all()
        if error is not None and not isinstance(error, Exception):
            raise error


class WindowStacker(_StackerFront):
    """Thread-safe front of one ``HipWindowGroup`` for the greedy steps (the queue: :class:`_StackerFront`): any thread
    hands its greedy window to :meth:`run`; the runner advances every window in flight with one ``step_pick`` per token
    and admits queued windows at its next step.  A window leaves at its end, the others go on.  A window the group refuses
    on the host (context full, no rules, ...) fails alone: the refused call advanced nobody, so the others take that step
    without it.

    ``solo_single``: while ONE window is in flight it takes the session's own step (``decode`` + ``pick_greedy``, a graph
    replay with the one-row folds) instead of a one-row group step, which measured 10 % slower; the two give
    the same token and the same log-probability bits on every input the tests step.

    ``burst`` (1..16, default ``WLK_TRANSCRIBE_STACK_BURST`` or 1): with more than 1, a pass over the windows in flight is
    ONE ``run_pick`` of up to that many tokens per window (``wlk_group_run_pick``): each window's budget is its
    ``steps_left``, the call is no longer than the longest budget, every row's picks are taken in order, and windows that
    arrive meanwhile are admitted before the next call.  With 1 the front calls ``step_pick`` as before."""

    def __init__(self, model, rows: int = 8, group=None, solo_single: bool = True, burst: Optional[int] = None):
        super().__init__(rows)
        self.burst = resolve_burst(burst)
        if group is None:
            from .engine import HipWindowGroup
            group = HipWindowGroup(model, self.rows)
        self.group = group
        self.solo_single = bool(solo_single)
        self.solo_steps = 0
        self.row_slots = 0             # rows x chains over the group calls: what is not in the group's `rows` went to dead rows

    def run(self, window: _GreedyWindow) -> None:
        """Advances ``window`` to its end (its tokens and sum are updated in place); raises what stopped it."""
        self.run_many([window])

    def _advance(self, live):
        return self._step(live)

    def _step(self, live: List[Tuple[int, _GreedyWindow]]) -> List[Tuple[int, _GreedyWindow]]:
        """one token (``burst`` > 1: up to that many) for every window in `live`; -> the windows still in flight"""
        burst = self.burst

        def step(part):
            if burst > 1:
                return self._burst(part, burst)
            ids, lps = self.group.step_pick([w.session for _t, w in part], [w.feed() for _t, w in part],
                                            [w.state() for _t, w in part])
            self.row_slots += len(part)
            return [(t, w) for (t, w), tok, lp in zip(part, ids, lps) if not self._taken(t, w, tok, lp)]
        if len(live) == 1 and self.solo_single:
            (t, w), = live
            try:                                   # whatever stops a window on its own chain is that window's own error
                w.session.decode(w.tokens[:, -1:], first=False)
                tok, lp = w.session.pick_greedy(**w.state())
            except Exception as e:
                self._settle(t, e)
                return []
            self.solo_steps += 1
            return [] if self._taken(t, w, tok, lp) else live
        try:
            return step(live)
        except Exception as e:
            if not _refused(e):
                raise
            if len(live) == 1:
                self._settle(live[0][0], e)
                return []
        keep = []
        for item in live:                          # the refused call advanced nobody: every window on its own
            try:
                keep += step([item])
            except Exception as e:
                if not _refused(e):
                    raise
                self._settle(item[0], e)
        return keep

    def _burst(self, part: List[Tuple[int, _GreedyWindow]], burst: int) -> List[Tuple[int, _GreedyWindow]]:
        """one ``run_pick`` for the windows of `part`: no chain is enqueued that no row can use"""
        budgets = [w.steps_left for _t, w in part]
        chains = min(burst, max(budgets))
        res = self.group.run_pick([w.session for _t, w in part], [w.feed() for _t, w in part],
                                  [w.state() for _t, w in part], budgets, chains)
        self.row_slots += len(part) * chains
        keep = []
        for (t, w), (ids, lps) in zip(part, res):
            over = False
            for tok, lp in zip(ids, lps):
                over = w.take(int(tok), float(lp))
            if over:
                self._settle(t, None)
            else:
                keep.append((t, w))
        return keep

    def _taken(self, ticket: int, window: _GreedyWindow, tok, lp) -> bool:
        if window.take(int(tok), float(lp)):
            self._settle(ticket, None)
            return True
        return False

    def stats(self) -> dict:
        """the group's steps (chains) and rows so far, and this front's passes, windows, solo steps and row slots (rows x
        chains of its group calls)"""
        return dict(self.group.stats(), passes=self.passes, windows=self.windows, solo_steps=self.solo_steps,
                    row_slots=self.row_slots)

    def close(self) -> None:
        self.group.close()


_STACK_LOCK = threading.Lock()


def set_stack(model, stack: Optional[int]) -> int:
    """Switches the stacked greedy windows of ``model`` on (1..8 rows) or off (0); ``None`` leaves it to
    ``WLK_TRANSCRIBE_STACK``.  -> the resolved value."""
    rows = resolve_stack(stack)
    with _STACK_LOCK:
        model.__dict__["_window_stack_rows"] = rows
    return rows


def set_burst(model, burst: Optional[int]) -> int:
    """Steps per library call of ``model``'s stacked greedy windows (1..16; 1 = one ``step_pick`` per token); ``None``
    leaves it to ``WLK_TRANSCRIBE_STACK_BURST``.  It only acts while the stacked windows are on (:func:`set_stack` /
    ``WLK_TRANSCRIBE_STACK`` >= 1).  -> the resolved value."""
    k = resolve_burst(burst)
    with _STACK_LOCK:
        if burst is None:
            model.__dict__.pop("_window_stack_burst", None)
        else:
            model.__dict__["_window_stack_burst"] = k
    return k


def _model_burst(model) -> int:
    k = model.__dict__.get("_window_stack_burst")
    return resolve_burst(None) if k is None else k


def window_stacker(model, rows: Optional[int] = None) -> Optional[WindowStacker]:
    """The model's stacker; created with ``rows`` rows when there is none yet (``rows`` None: never creates)."""
    with _STACK_LOCK:
        st = model.__dict__.get("_window_stacker")
        if st is None and rows:
            st = model.__dict__["_window_stacker"] = WindowStacker(model, rows)
        return st


def _with_model_burst(model, st):
    """the model's stacker with the model's burst (:func:`set_burst`, else ``WLK_TRANSCRIBE_STACK_BURST``) from its next pass on"""
    burst = _model_burst(model)
    if getattr(st, "burst", burst) != burst:
        st.burst = burst
    return st


def _run_stacker(model) -> Optional[WindowStacker]:
    """What `_WindowDecoder.run` sends its greedy steps through: the model's stacker when stacking is switched on for it
    (:func:`set_stack`, else ``WLK_TRANSCRIBE_STACK``), otherwise None - and then nothing is constructed.  The stacker takes
    the model's burst (:func:`set_burst`, else ``WLK_TRANSCRIBE_STACK_BURST``) from its next pass on."""
    rows = model.__dict__.get("_window_stack_rows")
    if rows is None:
        rows = resolve_stack(None)
    return _with_model_burst(model, window_stacker(model, rows)) if rows > 0 else None


# ---- stacked word alignment (opt-in; wlk_group_find_alignment) --------------------------------------------------------------
class _AlignWindow:
    """One window's word-alignment request: the encoded 1-row session, what :func:`timing.find_alignment` takes, and the
    WordTiming list once it is served."""

    def __init__(self, session, tokenizer, text_tokens: Sequence[int], num_frames: int):
        self.session, self.tokenizer = session, tokenizer
        self.text_tokens, self.num_frames = [int(t) for t in text_tokens], int(num_frames)
        self.result: Optional[list] = None

    def item(self) -> tuple:
        return (self.session, self.tokenizer, self.text_tokens, self.num_frames)


class AlignStacker(_StackerFront):
    """Thread-safe front of ``HipWindowGroup.find_alignment`` (the queue: :class:`_StackerFront`): any thread hands its
    window's alignment to :meth:`align`; the first caller drives, everything queued at that moment - up to the group's
    rows - is aligned by ONE stacked pass, windows that arrive during a pass ride the next one.  A window the group refuses
    on the host fails alone - the refused call touched nobody - and is then aligned by the solo ``timing.find_alignment``;
    the others go through without it.  A pass that fails otherwise hands its error to everyone in flight or queued.

    ``solo_single``: a window that is alone in its pass takes the solo ``timing.find_alignment`` instead of a group of
    one (DESIGN 27 says which was measured faster); both give the same words."""

    def __init__(self, model, rows: int = 8, group=None, solo_single: bool = False):
        super().__init__(rows)
        if group is None:
            from .engine import HipWindowGroup
            group = HipWindowGroup(model, self.rows)
        self.group = group
        self.solo_single = bool(solo_single)
        self.group_passes = 0          # stacked passes, and the windows they served
        self.stacked = 0
        self.solo = 0                  # windows served by the solo call (refused by the group, or alone with solo_single)

    def align(self, session, tokenizer, text_tokens: Sequence[int], num_frames: int) -> list:
        """-> the WordTiming list ``timing.find_alignment(session, tokenizer, text_tokens, None, num_frames)`` returns"""
        window = _AlignWindow(session, tokenizer, text_tokens, num_frames)
        self.run_many([window])
        return window.result

    def _solo(self, ticket: int, w: _AlignWindow) -> None:
        try:                                       # whatever stops a window on its own chain is that window's own error
            w.result = T.find_alignment(*w.item()[:3], None, w.num_frames)
            self.solo += 1
        except Exception as e:
            self._settle(ticket, e)
        else:
            self._settle(ticket, None)

    def _pass(self, part: list) -> None:
        results = T.find_alignment_many(self.group, [w.item() for _t, w in part])
        self.group_passes += 1
        self.stacked += len(part)
        for (t, w), res in zip(part, results):
            w.result = res
            self._settle(t, None)

    def _advance(self, live: list) -> list:
        if len(live) == 1 and self.solo_single:
            self._solo(*live[0])
            return []
        try:
            self._pass(live)
            return []
        except Exception as e:
            if not _refused(e):
                raise
        for item in live:                          # the refused call touched nobody: every window on its own
            try:
                self._pass([item])
            except Exception as e:
                if not _refused(e):
                    raise
                self._solo(*item)
        return []

    def stats(self) -> dict:
        """this front's drives and windows, the stacked passes with the windows they served, the solo windows"""
        return dict(passes=self.passes, windows=self.windows, group_passes=self.group_passes, stacked=self.stacked,
                    solo=self.solo, mean_windows_per_pass=round(self.stacked / self.group_passes, 3) if self.group_passes else None)


def resolve_align_stack(flag: Optional[bool]) -> bool:
    """``HipWhisperASR(align_stack=...)`` / :func:`set_align_stack`: an explicit value wins; ``None`` reads
    ``WLK_TRANSCRIBE_ALIGN_STACK`` (default off)."""
    if flag is None:
        return os.environ.get("WLK_TRANSCRIBE_ALIGN_STACK", "0").strip().lower() in ("1", "true", "on", "yes")
    return bool(flag)


def resolve_draft(flag: Optional[bool]) -> bool:
    """``HipWhisperASR(draft=...)``: an explicit value wins; ``None`` reads ``WLK_TRANSCRIBE_DRAFT`` (default off)."""
    if flag is None:
        return os.environ.get("WLK_TRANSCRIBE_DRAFT", "0").strip().lower() in ("1", "true", "on", "yes")
    return bool(flag)


def set_align_stack(model, flag: Optional[bool]) -> bool:
    """Switches the stacked word alignment of ``model`` on or off; ``None`` leaves it to ``WLK_TRANSCRIBE_ALIGN_STACK``.
    It only acts while the stacked windows are on as well (:func:`set_stack` / ``WLK_TRANSCRIBE_STACK`` >= 1).  -> the
    resolved value."""
    on = resolve_align_stack(flag)
    with _STACK_LOCK:
        if flag is None:
            model.__dict__.pop("_align_stack", None)
        else:
            model.__dict__["_align_stack"] = on
    return on


def align_stacker(model) -> Optional[AlignStacker]:
    """The model's alignment stacker, if one was ever constructed (never creates)."""
    with _STACK_LOCK:
        return model.__dict__.get("_align_stacker")


def _align_stacker(model) -> Optional[AlignStacker]:
    """What `_add_word_timestamps` sends a window's alignment through: the model's alignment stacker - over the
    :class:`WindowStacker`'s group - when both switches are on, otherwise None, and then nothing is constructed."""
    on = model.__dict__.get("_align_stack")
    if on is None:
        on = resolve_align_stack(None)
    if not on:
        return None
    windows = _run_stacker(model)
    if windows is None:
        return None
    with _STACK_LOCK:
        st = model.__dict__.get("_align_stacker")
        if st is None:
            st = model.__dict__["_align_stacker"] = AlignStacker(model, windows.rows, group=windows.group)
        return st


def _tokenizer_for(model: HipWhisperModel, language: Optional[str], task: Optional[str]) -> WhisperTokenizer:
    return get_tokenizer(model.is_multilingual, num_languages=model.num_languages, language=language, task=task)


def _logits(session: HipSession, rows: int, n_vocab: int, what: str = "logits_last") -> np.ndarray:
    session.sync()
    return session.export(what, rows * n_vocab).reshape(rows, n_vocab)


def _logsumexp(x: np.ndarray) -> np.float32:
    m = x.max()
    if not np.isfinite(m):
        return np.float32(m)
    return np.float32(m + np.log(np.exp(x - m).sum(dtype=np.float32)))


def _log_softmax(x: np.ndarray) -> np.ndarray:
    """F.log_softmax(logits.float(), dim=-1) row by row, single-threaded."""
    m = x.max(axis=-1, keepdims=True)
    z = x - m
    return z - np.log(np.exp(z).sum(axis=-1, keepdims=True, dtype=np.float32))


# ---- language id (decoding.py:19-77) ----------------------------------------------------------------------------------------
def detect_language(model: HipWhisperModel, mel: Optional[np.ndarray], tokenizer: Optional[WhisperTokenizer] = None,
                    *, session: Optional[HipSession] = None) -> Tuple[int, Dict[str, float]]:
    """-> (most probable language token, {code: probability}).  ``mel`` None: the session is already encoded."""
    if tokenizer is None:
        tokenizer = _tokenizer_for(model, None, None)
    if tokenizer.language is None or (tokenizer.sot + 1 + tokenizer.all_language_codes.index(tokenizer.language)
                                      not in tokenizer.sot_sequence):
        raise ValueError("This model doesn't have language tokens so it can't perform lang id")
    s = session or _rows_of(model).get(1)
    if mel is not None:
        s.encode_mel(pad_or_trim(np.asarray(mel)))
    rows = s.beam
    s.decode(np.full((rows, 1), tokenizer.sot, np.int64), first=True, sot_index=0)
    logits = torch.from_numpy(_logits(s, rows, model.dims.n_vocab)[0])
    keep = torch.zeros(logits.shape[-1], dtype=torch.bool)
    keep[list(tokenizer.all_language_tokens)] = True
    logits[~keep] = NEG_INF
    token = int(logits.argmax())
    probs = logits.softmax(dim=-1)
    return token, {c: float(probs[t]) for t, c in zip(tokenizer.all_language_tokens, tokenizer.all_language_codes)}


# ---- one 30 s window (decoding.py:502-784) ----------------------------------------------------------------------------------
class _WindowDecoder:
    def __init__(self, model: HipWhisperModel, options: DecodingOptions):
        self.model = model
        self.o = options
        self._check(options)
        self.tok = _tokenizer_for(model, options.language or "en", options.task)
        d = model.dims
        self.n_group = options.beam_size or options.best_of or 1
        self.n_ctx = d.n_text_ctx
        self.sample_len = options.sample_len or d.n_text_ctx // 2
        self.sot_sequence = (self.tok.sot_sequence_including_notimestamps if options.without_timestamps
                             else self.tok.sot_sequence)
        self.initial = self._initial_tokens()
        self.sample_begin = len(self.initial)
        self.sot_index = self.initial.index(self.tok.sot)
        self.blank_ids = [*self.tok.encode(" "), self.tok.eot] if options.suppress_blank else None
        self.suppressed = self._suppressed() if options.suppress_tokens else None
        self.max_initial_ts = None
        if not options.without_timestamps and options.max_initial_timestamp:
            self.max_initial_ts = round(options.max_initial_timestamp / (CHUNK_LENGTH / d.n_audio_ctx))

    @staticmethod
    def _check(o: DecodingOptions) -> None:
        if o.beam_size is not None and o.best_of is not None:
            raise ValueError("beam_size and best_of can't be given together")
        if o.temperature == 0 and o.best_of is not None:
            raise ValueError("best_of with greedy sampling (T=0) is not compatible")
        if o.patience is not None and o.beam_size is None:
            raise ValueError("patience requires beam_size to be given")
        if o.length_penalty is not None and not 0 <= o.length_penalty <= 1:
            raise ValueError("length_penalty (alpha) should be a value between 0 and 1")

    def _as_ids(self, text_or_ids) -> List[int]:
        return self.tok.encode(" " + text_or_ids.strip()) if isinstance(text_or_ids, str) else list(text_or_ids)

    def _initial_tokens(self) -> List[int]:
        """[<|startofprev|>, last n_ctx/2 - 1 prompt ids] + sot sequence + prefix (decoding.py:581-607)."""
        ids = list(self.sot_sequence)
        if self.o.prefix:
            prefix = self._as_ids(self.o.prefix)
            if self.sample_len is not None:
                room = self.n_ctx // 2 - self.sample_len
                prefix = prefix[-room:]          # room == 0 keeps everything, as in the reference
            ids = ids + prefix
        if self.o.prompt:
            prompt = self._as_ids(self.o.prompt)
            ids = [self.tok.sot_prev] + prompt[-(self.n_ctx // 2 - 1):] + ids
        return ids

    def _suppressed(self) -> List[int]:
        """decoding.py:609-636: "-1" = the tokenizer's annotation symbols; always the task / sot family and <|nospeech|>."""
        sup = self.o.suppress_tokens
        if isinstance(sup, str):
            sup = [int(t) for t in sup.split(",")]
        sup = list(sup)
        if -1 in sup:
            sup = [t for t in sup if t >= 0] + list(self.tok.non_speech_tokens)
        t = self.tok
        sup += [t.transcribe, t.translate, t.sot, t.sot_prev, t.sot_lm]
        if t.no_speech is not None:
            sup.append(t.no_speech)
        return sorted(set(sup))

    # -- logit rules (decoding.py:417-499), in the reference's order ------------------------------------------------------
    def _apply_rules(self, logits: np.ndarray, tokens: np.ndarray) -> np.ndarray:
        """In place on the [rows, vocabulary] logits; -> log_softmax of the result.  numpy on purpose: these are
        reductions over one 50k-element row per step, and torch's CPU operators hand such a row to the whole intra-op
        thread pool (3 ms per call on a 128-thread host against 0.1 ms single-threaded)."""
        tb, eot = self.tok.timestamp_begin, self.tok.eot
        first_step = tokens.shape[1] == self.sample_begin
        if self.blank_ids is not None and first_step:
            logits[:, self.blank_ids] = NEG_INF
        if self.suppressed is not None:
            logits[:, self.suppressed] = NEG_INF
        if self.o.without_timestamps:
            return _log_softmax(logits)
        if self.tok.no_timestamps is not None:
            logits[:, self.tok.no_timestamps] = NEG_INF
        for k in range(tokens.shape[0]):
            sampled = tokens[k, self.sample_begin:]
            last_ts = len(sampled) >= 1 and sampled[-1] >= tb
            before_last_ts = len(sampled) < 2 or sampled[-2] >= tb
            if last_ts:
                if before_last_ts:
                    logits[k, tb:] = NEG_INF            # a closed pair: text (or <|endoftext|>) must follow
                else:
                    logits[k, :eot] = NEG_INF           # an opening timestamp needs its partner (or the end)
            stamps = sampled[sampled >= tb]
            if len(stamps) > 0:
                # never backwards; and strictly forwards unless this closes a segment (no zero-length loops)
                bound = int(stamps[-1]) if (last_ts and not before_last_ts) else int(stamps[-1]) + 1
                logits[k, tb:bound] = NEG_INF
        if first_step:
            logits[:, :tb] = NEG_INF                    # a window opens with a timestamp ...
            if self.max_initial_ts is not None:
                logits[:, tb + self.max_initial_ts + 1:] = NEG_INF      # ... no later than max_initial_timestamp
        logprobs = _log_softmax(logits)
        changed = False
        for k in range(tokens.shape[0]):
            if _logsumexp(logprobs[k, tb:]) > logprobs[k, :tb].max():
                logits[k, :tb] = NEG_INF                # timestamps as a group outweigh every text token
                changed = True
        return _log_softmax(logits) if changed else logprobs

    def _pick_states(self, tokens: np.ndarray) -> List[dict]:
        """What ApplyTimestampRules (decoding.py:441-499) reads from the sampled tokens of every row, as the fields of
        wlk_pick_params: the device applies the rules to the logits rows, the histories stay here."""
        tb = self.tok.timestamp_begin
        states = []
        for row in tokens:
            sampled = row[self.sample_begin:]
            last_ts = len(sampled) >= 1 and sampled[-1] >= tb
            before_last_ts = len(sampled) < 2 or sampled[-2] >= tb
            stamps = sampled[sampled >= tb]
            bound = tb
            if len(stamps) > 0:
                bound = int(stamps[-1]) if (last_ts and not before_last_ts) else int(stamps[-1]) + 1
            states.append(dict(first_step=tokens.shape[1] == self.sample_begin,
                               without_timestamps=bool(self.o.without_timestamps), timestamp_begin=tb, eot=self.tok.eot,
                               no_timestamps=-1 if self.tok.no_timestamps is None else int(self.tok.no_timestamps),
                               ts_mode=0 if not last_ts else (1 if before_last_ts else 2), ts_bound=bound,
                               max_initial=-1 if self.max_initial_ts is None else int(self.max_initial_ts)))
        return states

    def _pick_state(self, tokens: np.ndarray) -> dict:
        """The one sequence of the greedy loop: row 0 of `_pick_states`."""
        return self._pick_states(tokens[:1])[0]

    # -- draft verification --------------------------------------------------------------------------------
    def draft_window(self, session, initial: Sequence[int], group) -> Optional[tuple]:
        """The ``HipWindowGroup.verify`` window of this decoder's draft behind ``initial`` in ``session`` (encoded, rules
        set), or None: no draft is left after clamping, or the range is outside the stacked pass."""
        draft = clamp_draft(self.o.draft, len(initial), self.sample_len, self.n_ctx, self.tok.eot)
        if not draft or not group.verify_fits(len(initial), len(draft)):
            return None
        state = self._pick_state(np.asarray([list(initial)], np.int64))
        return (session, list(initial), draft, self.sot_index, state, self.tok.no_speech)

    def takes_draft(self, session) -> bool:
        """the conditions of `run`'s device-rules greedy path, for a caller (`decode_many`) that verifies ahead of `run`"""
        o = self.o
        return (o.draft is not None and o.beam_size is None and self.n_group == 1 and o.temperature == 0
                and o.language is not None and o.task != "lang_id" and hasattr(session, "pick_greedy")
                and os.environ.get("WLK_TRANSCRIBE_DEVICE_RULES", "1") != "0")

    def set_rules(self, session) -> None:
        session.set_rules(self.suppressed or [], self.blank_ids or [])

    # -- the loop ------------------------------------------------------------------------------------------------------
    def run(self, mel_segment: Optional[np.ndarray], session: Optional[HipSession] = None, *,
            stacker: Optional[WindowStacker] = None, defer: bool = False, verified: Optional[dict] = None):
        """-> the window's DecodingResult.  ``stacker``: the greedy temperature-0 steps behind the first pick go through it
        (default: the model's, when stacking is switched on).  ``defer`` (`decode_many`): a window that reaches those steps
        comes back as ``(_GreedyWindow, finish)`` instead - the caller advances it and calls ``finish()`` for the result.
        ``verified`` (`decode_many`): what ``HipWindowGroup.verify`` returned for this window's `draft_window`, with that
        window's draft under the key ``draft`` - the session is encoded and verified already."""
        o, tok, V = self.o, self.tok, self.model.dims.n_vocab
        rows = self.n_group
        s = session or _rows_of(self.model).get(rows)
        if mel_segment is not None:
            s.encode_mel(pad_or_trim(np.asarray(mel_segment)))
        initial = list(self.initial)
        language, language_probs = o.language, None
        if o.language is None or o.task == "lang_id":
            lang_token, language_probs = detect_language(self.model, None, tok, session=s)
            language = max(language_probs, key=language_probs.get)
            if o.language is None:
                initial[self.sot_index + 1] = lang_token
            if o.task == "lang_id":
                return DecodingResult(language=language, language_probs=language_probs)

        tokens = np.tile(np.asarray(initial, np.int64), (rows, 1))
        sum_logprobs = np.zeros(rows, np.float32)
        no_speech = float("nan")
        beam = BeamUpdate(o.beam_size, tok.eot, o.patience or 1.0) if o.beam_size is not None else None
        if beam is not None and beam.max_candidates <= 0:
            raise ValueError(f"Invalid beam size ({o.beam_size}) or patience ({o.patience})")
        # greedy decoding of one sequence at temperature 0: rules, argmax and log-probability on the device, 8 bytes back per
        # step (WLK_TRANSCRIBE_DEVICE_RULES=0: the host path below, which sampling and beam search always take)
        device_rules = (beam is None and rows == 1 and o.temperature == 0 and hasattr(s, "pick_greedy")
                        and os.environ.get("WLK_TRANSCRIBE_DEVICE_RULES", "1") != "0")
        # beam search (2..7 beams) at temperature 0 with WLK_TRANSCRIBE_DEVICE_BEAM=1: rules, log-softmax and the beam + 1 best
        # of every row on the device (beam * (beam + 1) pairs back per step), and single-token steps that read the
        # self-attention cache through the ancestry table instead of gathering it.  Off by default.
        device_beam = (beam is not None and 2 <= o.beam_size <= 7 and o.temperature == 0 and hasattr(s, "pick_topk")
                       and os.environ.get("WLK_TRANSCRIBE_DEVICE_BEAM", "0") == "1")
        if device_rules or device_beam:
            self.set_rules(s)
        if device_rules and stacker is None:
            stacker = _run_stacker(self.model)
        stacked = stacker if device_rules else None

        def finish(tokens=None, sum_logprobs=None, window: Optional[_GreedyWindow] = None) -> DecodingResult:
            # candidates of the group (decoding.py:289-292 / :378-399), cut between the first sampled token and <|endoftext|>
            if window is not None:
                tokens, sum_logprobs = window.tokens, window.sum_logprobs
            if beam is not None:
                finished = beam.finished[0]
                if len(finished) < o.beam_size:
                    for j in np.argsort(sum_logprobs)[::-1]:
                        finished[tuple(tokens[j].tolist() + [tok.eot])] = float(sum_logprobs[j])
                        if len(finished) >= o.beam_size:
                            break
                candidates = [list(seq) for seq in finished]
                sums = [float(v) for v in finished.values()]
            else:
                candidates = [row.tolist() + [tok.eot] for row in tokens]
                sums = [float(v) for v in sum_logprobs]
            candidates = [c[self.sample_begin:c.index(tok.eot)] for c in candidates]
            best = self._rank(candidates, sums)
            out = candidates[best]
            text = tok.decode(out).strip()
            return DecodingResult(language=language, language_probs=language_probs, tokens=out, text=text,
                                  avg_logprob=sums[best] / (len(out) + 1), no_speech_prob=no_speech,
                                  temperature=o.temperature, compression_ratio=compression_ratio(text))

        if stacked is not None and verified is None and o.draft is not None:
            # ONE teacher-forced pass over [initial | draft] instead of the prefill, the first pick and a step per
            # accepted token; a range the group refuses on the host (nothing launched, the session untouched) and an
            # unusable draft take the statements below
            win = self.draft_window(s, initial, stacked.group)
            if win is not None:
                try:
                    verified = dict(stacked.group.verify([win])[0], draft=win[2])
                except Exception as e:
                    if not _refused(e):
                        raise
        if stacked is not None and verified is not None:
            k = int(verified["accepted"])
            taken = initial + [int(t) for t in verified["draft"][:k]] + [int(verified["next_token"])]
            tokens = np.asarray([taken], np.int64)
            sum_logprobs[0] = np.float32(verified["sum_logprob"])
            if tok.no_speech is not None:
                no_speech = float(verified["no_speech_prob"])
            # the loop below, entered behind its iteration k: k + 1 tokens are sampled
            if tokens[0, -1] == tok.eot or tokens.shape[-1] > self.n_ctx or k + 1 >= self.sample_len:
                return finish(tokens, sum_logprobs)
            window = _GreedyWindow(self, s, tokens, sum_logprobs, self.sample_len - 1 - k)
            if defer:
                return window, lambda: finish(window=window)
            stacked.run(window)
            return finish(window=window)

        sources = None
        for i in range(self.sample_len):
            if device_beam and i > 0:
                s.decode_ancestry(tokens[:, -1], sources)
            else:
                s.decode(tokens if i == 0 else tokens[:, -1:], first=(i == 0), sot_index=self.sot_index)
            if i == 0 and tok.no_speech is not None:
                no_speech = float(s.no_speech_prob(tok.no_speech)[0])
            if device_beam:
                top_lp, top_id = s.pick_topk(self._pick_states(tokens), o.beam_size + 1)
                tokens, done, sources = beam.update(tokens, top_lp, top_id, sum_logprobs)
                if done or tokens.shape[-1] > self.n_ctx:
                    break
                continue
            if device_rules:
                nxt_id, picked = s.pick_greedy(**self._pick_state(tokens))
                tokens, over = _greedy_take(tokens, sum_logprobs, nxt_id, picked, tok.eot, self.n_ctx)
                if over:
                    break
                if stacked is not None and i + 1 < self.sample_len:
                    # the prefill and its pick were this session's own; every further step rides in the group
                    window = _GreedyWindow(self, s, tokens, sum_logprobs, self.sample_len - 1 - i)
                    if defer:
                        return window, lambda: finish(window=window)
                    stacked.run(window)
                    return finish(window=window)
                continue
            logits = _logits(s, rows, V)
            logprobs = self._apply_rules(logits, tokens)
            if beam is not None:
                top_lp, top_id = torch.from_numpy(logprobs).topk(o.beam_size + 1, dim=-1)
                tokens, done, sources = beam.update(tokens, top_lp.numpy(), top_id.numpy(), sum_logprobs)
                s.kv_reorder(sources)
            else:
                nxt = choose(torch.from_numpy(logits), o.temperature)
                picked = logprobs[np.arange(rows), nxt.numpy()]
                live = tokens[:, -1] != tok.eot
                sum_logprobs += picked * live
                nxt = np.where(live, nxt.numpy(), tok.eot)
                tokens = np.concatenate([tokens, nxt[:, None].astype(np.int64)], axis=1)
                done = bool((tokens[:, -1] == tok.eot).all())
            if done or tokens.shape[-1] > self.n_ctx:
                break

        return finish(tokens, sum_logprobs)

    def _rank(self, candidates: List[List[int]], sums: List[float]) -> int:
        """MaximumLikelihoodRanker (decoding.py:184-207): log-probability over length, or over ((5 + length) / 6) ** alpha."""
        def norm(n):
            return n if self.o.length_penalty is None else ((5 + n) / 6) ** self.o.length_penalty
        return int(np.argmax([lp / norm(len(c)) for c, lp in zip(candidates, sums)]))


def decode(model: HipWhisperModel, mel: Optional[np.ndarray], options: DecodingOptions = DecodingOptions(), *,
           session: Optional[HipSession] = None, stacker: Optional[WindowStacker] = None, **kwargs) -> DecodingResult:
    """decoding.py:787-820 for one 30 s segment [n_mels, 3000] (None: the session already holds the encoded window).
    ``stacker``: the window stacker of the greedy temperature-0 steps (default: the model's, when stacking is switched on);
    ``options.draft`` acts only where there is one."""
    if kwargs:
        options = replace(options, **kwargs)
    return _WindowDecoder(model, options).run(mel, session, stacker=stacker)


def decode_many(model: HipWhisperModel, mels: Sequence[np.ndarray], options: DecodingOptions = DecodingOptions(), *,
                stacker: Optional[WindowStacker] = None, drafts: Optional[Sequence[Optional[Sequence[int]]]] = None,
                **kwargs) -> List[DecodingResult]:
    """decoding.py:787-820 for up to 8 segments [n, n_mels, 3000] at once, greedy at temperature 0: one result per window,
    in order.  Encoder, language detection, prefill, first pick and no-speech probability are each window's own (one
    session per window); from there every token of all windows still alive is ONE ``HipWindowGroup.step_pick``.  A window
    leaves at <|endoftext|>, at sample_len or at n_ctx; the others go on.  ``drafts`` (one entry per window, None = none):
    after their encodes, the windows with a usable draft open with ONE ``HipWindowGroup.verify`` for all of them instead of
    a prefill and a first pick each; the others open as before."""
    if kwargs:
        options = replace(options, **kwargs)
    if options.temperature != 0 or options.beam_size is not None or options.best_of is not None:
        raise ValueError("decode_many decodes greedily at temperature 0 (sampling and beam search: decode())")
    mels = [np.asarray(m) for m in mels]
    if not 1 <= len(mels) <= 8:
        raise ValueError("decode_many takes 1..8 windows")
    if drafts is not None and len(drafts) != len(mels):
        raise ValueError("decode_many: one draft (or None) per window")
    if stacker is None:
        stacker = _with_model_burst(model, window_stacker(model, 8))
    sessions =_rows_of(model).windows(len(mels))
    if drafts is not None and any(d is not None for d in drafts):
        return _decode_many_drafts(model, mels, sessions, options, stacker, drafts)
    opened = [_WindowDecoder(model, options).run(mel, s, stacker=stacker, defer=True) for mel, s in zip(mels, sessions)]
    stacker.run_many([r[0] for r in opened if isinstance(r, tuple)])
    return [r[1]() if isinstance(r, tuple) else r for r in opened]


def _decode_many_drafts(model, mels, sessions, options, stacker, drafts) -> List[DecodingResult]:
    """`decode_many` with drafts: every window is encoded first, the windows with a usable draft share one verify pass, then
    each window opens (from its verify result, or with its own prefill and first pick) and all go on in the stacker."""
    decoders = [_WindowDecoder(model, replace(options, draft=d)) for d in drafts]
    windows: List[Optional[tuple]] = []
    for dec, mel, s in zip(decoders, mels, sessions):
        s.encode_mel(pad_or_trim(mel))
        win = None
        if dec.takes_draft(s):
            dec.set_rules(s)
            win = dec.draft_window(s, dec.initial, stacker.group)
        windows.append(win)
    verified: List[Optional[dict]] = [None] * len(mels)
    riding = [i for i, w in enumerate(windows) if w is not None]
    if riding:
        try:
            for i, res in zip(riding, stacker.group.verify([windows[i] for i in riding])):
                verified[i] = dict(res, draft=windows[i][2])
        except Exception as e:                     # refused on the host: nothing was launched, every window opens on its own
            if not _refused(e):
                raise
    # a window without a verify result still carries its draft into `run`, which then tries it alone (a refusal of the
    # joint call may have been another window's)
    opened = [dec.run(None, s, stacker=stacker, defer=True, verified=v) for dec, s, v in zip(decoders, sessions, verified)]
    stacker.run_many([r[0] for r in opened if isinstance(r, tuple)])
    return [r[1]() if isinstance(r, tuple) else r for r in opened]


# ---- the window loop (transcribe.py:21-494) ---------------------------------------------------------------------------------
_PUNCTUATION = "\"'“¿([{-\"'.。,，!！?？:：”)]}、"


def _word_anomaly(word: dict) -> float:
    """transcribe.py:287-297: improbable, very short or very long words score."""
    duration = word["end"] - word["start"]
    score = 1.0 if word.get("probability", 0.0) < 0.15 else 0.0
    if duration < 0.133:
        score += (0.133 - duration) * 15
    if duration > 2.0:
        score += duration - 2.0
    return score


def _segment_is_anomaly(segment: Optional[dict]) -> bool:
    if segment is None or not segment["words"]:
        return False
    words = [w for w in segment["words"] if w["word"] not in _PUNCTUATION][:8]
    score = sum(_word_anomaly(w) for w in words)
    return score >= 3 or score + 0.01 >= len(words)


def _first_with_words(segments: Sequence[dict]) -> Optional[dict]:
    return next((s for s in segments if s["words"]), None)


def _last_word_end(segments: Sequence[dict]) -> Optional[float]:
    """utils.py:78-82."""
    for seg in reversed(segments):
        for w in reversed(seg["words"]):
            return w["end"]
    return segments[-1]["end"] if segments else None


def transcribe(model: HipWhisperModel, audio, *, verbose: Optional[bool] = None,
               temperature: Union[float, Tuple[float, ...]] = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0),
               compression_ratio_threshold: Optional[float] = 2.4, logprob_threshold: Optional[float] = -1.0,
               no_speech_threshold: Optional[float] = 0.6, condition_on_previous_text: bool = True,
               initial_prompt: Optional[str] = None, carry_initial_prompt: bool = False, word_timestamps: bool = False,
               prepend_punctuations: str = T.PREPEND_PUNCTUATIONS, append_punctuations: str = T.APPEND_PUNCTUATIONS,
               clip_timestamps: Union[str, List[float]] = "0", hallucination_silence_threshold: Optional[float] = None,
               draft: Optional[WindowDraft] = None, **decode_options) -> dict:
    """-> {"text", "segments": [{"id", "seek", "start", "end", "text", "tokens", "temperature", "avg_logprob",
    "compression_ratio", "no_speech_prob", ("words")}], "language"}.

    ``draft`` (not in the reference): one session's memory across the calls on its growing buffer.  The first
    window of the call (seek 0) at the first temperature of the ladder, when that is 0, verifies the tokens the same
    window sampled in the previous call, provided this call's audio begins with that call's audio; on return the memory
    holds this call's audio and first window.  Fallback temperatures, later windows, beam search and sampling never see
    it, and the result is the one the call gives without it."""
    if isinstance(audio, str):
        raise TypeError("transcribe: pass samples (float32, 16 kHz); decoding a file is outside the accelerated path")
    if hasattr(audio, "detach"):
        audio = audio.detach().cpu().numpy()
    audio = np.ascontiguousarray(audio, dtype=np.float32).reshape(-1)
    decode_options = dict(decode_options)
    decode_options["fp16"] = False
    draft_tokens = draft.begin(audio) if draft is not None else []
    dims = model.dims
    session = _rows_of(model).get(1)

    mel = session.log_mel(audio, padding=N_SAMPLES)            # 30 s of silence appended, for slicing
    content_frames = mel.shape[-1] - N_FRAMES
    content_duration = float(content_frames * HOP_LENGTH / SAMPLE_RATE)

    if decode_options.get("language") is None:
        if not model.is_multilingual:
            decode_options["language"] = "en"
        else:
            if verbose:
                print("Detecting language using up to the first 30 seconds. Use `--language` to specify the language")
            _, probs = detect_language(model, pad_or_trim(mel), session=session)
            decode_options["language"] = max(probs, key=probs.get)
            if verbose is not None:
                print(f"Detected language: {decode_options['language']}")
    language: str = decode_options["language"]
    task: str = decode_options.get("task", "transcribe")
    tokenizer = _tokenizer_for(model, language, task)

    if isinstance(clip_timestamps, str):
        clip_timestamps = [float(ts) for ts in (clip_timestamps.split(",") if clip_timestamps else [])]
    points = [round(ts * FRAMES_PER_SECOND) for ts in clip_timestamps]
    if not points:
        points.append(0)
    if len(points) % 2 == 1:
        points.append(content_frames)
    clips = list(zip(points[::2], points[1::2]))

    if word_timestamps and task == "translate":
        warnings.warn("Word-level timestamps on translations may not be reliable.")

    temperatures = [temperature] if isinstance(temperature, (int, float)) else list(temperature)

    def decode_with_fallback(segment: np.ndarray, window_draft: Optional[List[int]] = None) -> DecodingResult:
        result = None
        for n, t in enumerate(temperatures):
            kw = dict(decode_options)
            if window_draft and n == 0 and t == 0 and kw.get("beam_size") is None:
                kw["draft"] = window_draft
            if t > 0:
                kw.pop("beam_size", None)         # sampling: no beam
                kw.pop("patience", None)
            else:
                kw.pop("best_of", None)           # greedy / beam: no best_of
            opts = DecodingOptions(**kw, temperature=t)
            rows = opts.beam_size or opts.best_of or 1
            sess = _rows_of(model).get(rows)
            # the encoder output of this window stays in the session across the temperatures
            result = _WindowDecoder(model, opts).run(segment if (n == 0 or sess is not encoded_in[0]) else None, sess)
            encoded_in[0] = sess
            retry = False
            if compression_ratio_threshold is not None and result.compression_ratio > compression_ratio_threshold:
                retry = True                      # too repetitive
            if logprob_threshold is not None and result.avg_logprob < logprob_threshold:
                retry = True                      # too improbable
            if (no_speech_threshold is not None and result.no_speech_prob > no_speech_threshold
                    and logprob_threshold is not None and result.avg_logprob < logprob_threshold):
                retry = False                     # silence: improbable text is expected
            if not retry:
                break
        return result

    encoded_in: List[Optional[HipSession]] = [None]
    input_stride = N_FRAMES // dims.n_audio_ctx                      # mel frames per encoder position: 2
    assert N_FRAMES % dims.n_audio_ctx == 0
    time_precision = input_stride * HOP_LENGTH / SAMPLE_RATE         # 0.02 s
    all_tokens: List[int] = []
    all_segments: List[dict] = []
    prompt_reset_since = 0
    remaining_prompt_length = dims.n_text_ctx // 2 - 1
    if initial_prompt is not None:
        initial_prompt_tokens = tokenizer.encode(" " + initial_prompt.strip())
        all_tokens.extend(initial_prompt_tokens)
        remaining_prompt_length -= len(initial_prompt_tokens)
    else:
        initial_prompt_tokens = []

    ts_begin = tokenizer.timestamp_begin
    last_speech_timestamp = 0.0
    clip_idx = 0
    seek = clips[0][0]
    n_windows = 0
    while clip_idx < len(clips):
        clip_start, clip_end = clips[clip_idx]
        if seek < clip_start:
            seek = clip_start
        if seek >= clip_end:
            clip_idx += 1
            if clip_idx < len(clips):
                seek = clips[clip_idx][0]
            continue
        time_offset = float(seek * HOP_LENGTH / SAMPLE_RATE)
        window_end_time = float((seek + N_FRAMES) * HOP_LENGTH / SAMPLE_RATE)
        segment_size = min(N_FRAMES, content_frames - seek, clip_end - seek)
        segment_duration = segment_size * HOP_LENGTH / SAMPLE_RATE
        mel_segment = pad_or_trim(mel[:, seek:seek + segment_size])

        if carry_initial_prompt:
            ignored = max(len(initial_prompt_tokens), prompt_reset_since)
            decode_options["prompt"] = initial_prompt_tokens + all_tokens[ignored:][-remaining_prompt_length:]
        else:
            decode_options["prompt"] = all_tokens[prompt_reset_since:]

        encoded_in[0] = None
        first_window = draft is not None and n_windows == 0 and seek == 0
        n_windows += 1
        result = decode_with_fallback(mel_segment, draft_tokens if first_window else None)
        if first_window:
            draft.remember(result.tokens)
        tokens = np.asarray(result.tokens, dtype=np.int64)

        if no_speech_threshold is not None:
            skip = result.no_speech_prob > no_speech_threshold
            if logprob_threshold is not None and result.avg_logprob > logprob_threshold:
                skip = False                      # confident text despite the no-speech probability
            if skip:
                seek += segment_size
                continue

        previous_seek = seek
        current: List[dict] = []

        def new_segment(start: float, end: float, ids: np.ndarray) -> dict:
            ids = [int(t) for t in ids]
            return {"seek": seek, "start": start, "end": end,
                    "text": tokenizer.decode([t for t in ids if t < tokenizer.eot]), "tokens": ids,
                    "temperature": result.temperature, "avg_logprob": result.avg_logprob,
                    "compression_ratio": result.compression_ratio, "no_speech_prob": result.no_speech_prob}

        is_ts = tokens >= ts_begin
        single_timestamp_ending = is_ts[-2:].tolist() == [False, True]
        pair_ends = (np.where(is_ts[:-1] & is_ts[1:])[0] + 1).tolist()
        if pair_ends:
            # consecutive timestamp tokens close one segment and open the next
            if single_timestamp_ending:
                pair_ends.append(len(tokens))
            lo = 0
            for hi in pair_ends:
                piece = tokens[lo:hi]
                current.append(new_segment(time_offset + (int(piece[0]) - ts_begin) * time_precision,
                                           time_offset + (int(piece[-1]) - ts_begin) * time_precision, piece))
                lo = hi
            if single_timestamp_ending:
                seek += segment_size              # nothing is spoken after the last timestamp
            else:
                seek += (int(tokens[lo - 1]) - ts_begin) * input_stride     # redo the unfinished tail
        else:
            duration = segment_duration
            stamps = tokens[is_ts]
            if len(stamps) > 0 and int(stamps[-1]) != ts_begin:
                duration = (int(stamps[-1]) - ts_begin) * time_precision
            current.append(new_segment(time_offset, time_offset + duration, tokens))
            seek += segment_size

        if word_timestamps:
            _add_word_timestamps(current, session if encoded_in[0] is session else None, model, tokenizer, mel_segment,
                                 segment_size, prepend_punctuations, append_punctuations, last_speech_timestamp)
            if not single_timestamp_ending:
                end = _last_word_end(current)
                if end is not None and end > time_offset:
                    seek = round(end * FRAMES_PER_SECOND)

            if hallucination_silence_threshold is not None:
                threshold = hallucination_silence_threshold
                if not single_timestamp_ending:
                    end = _last_word_end(current)
                    if end is not None and end > time_offset:
                        seek = (round(end * FRAMES_PER_SECOND) if window_end_time - end > threshold
                                else previous_seek + segment_size)
                # a doubtful first segment: skip the silence before it and decode again from there
                first = _first_with_words(current)
                if first is not None and _segment_is_anomaly(first):
                    gap = first["start"] - time_offset
                    if gap > threshold:
                        seek = previous_seek + round(gap * FRAMES_PER_SECOND)
                        continue
                # a doubtful segment with silence (or more doubt) on both sides: drop it and what follows
                hal_last_end = last_speech_timestamp
                for si, segment in enumerate(current):
                    if not segment["words"]:
                        continue
                    if _segment_is_anomaly(segment):
                        following = _first_with_words(current[si + 1:])
                        hal_next_start = (following["words"][0]["start"] if following is not None
                                          else time_offset + segment_duration)
                        silence_before = (segment["start"] - hal_last_end > threshold or segment["start"] < threshold
                                          or segment["start"] - time_offset < 2.0)
                        silence_after = (hal_next_start - segment["end"] > threshold or _segment_is_anomaly(following)
                                         or window_end_time - segment["end"] < 2.0)
                        if silence_before and silence_after:
                            seek = round(max(time_offset + 1, segment["start"]) * FRAMES_PER_SECOND)
                            if content_duration - segment["end"] < threshold:
                                seek = content_frames
                            current[si:] = []
                            break
                    hal_last_end = segment["end"]

            end = _last_word_end(current)
            if end is not None:
                last_speech_timestamp = end

        if verbose:
            for segment in current:
                print(f"[{_stamp(segment['start'])} --> {_stamp(segment['end'])}] {segment['text']}")

        for segment in current:                   # instantaneous or empty segments keep their slot, without content
            if segment["start"] == segment["end"] or segment["text"].strip() == "":
                segment["text"] = ""
                segment["tokens"] = []
                segment["words"] = []

        all_segments.extend({"id": i, **segment} for i, segment in enumerate(current, start=len(all_segments)))
        all_tokens.extend(t for segment in current for t in segment["tokens"])
        if not condition_on_previous_text or result.temperature > 0.5:
            prompt_reset_since = len(all_tokens)  # text sampled at a high temperature is not fed back

    return dict(text=tokenizer.decode(all_tokens[len(initial_prompt_tokens):]), segments=all_segments, language=language)


def _stamp(seconds: float) -> str:
    ms = round(seconds * 1000.0)
    h, ms = divmod(ms, 3_600_000)
    m, ms = divmod(ms, 60_000)
    s, ms = divmod(ms, 1_000)
    return (f"{h:02d}:" if h else "") + f"{m:02d}:{s:02d}.{ms:03d}"


def _add_word_timestamps(segments: List[dict], encoded: Optional[HipSession], model: HipWhisperModel,
                         tokenizer: WhisperTokenizer, mel_segment: np.ndarray, num_frames: int, prepend: str, append: str,
                         last_speech_timestamp: float) -> None:
    """timing.py:279-388: one alignment pass over the text of all segments of the window, dealt back to them."""
    if not segments:
        return
    per_segment = [[t for t in seg["tokens"] if t < tokenizer.eot] for seg in segments]
    text_tokens = [t for ids in per_segment for t in ids]
    if encoded is None:                           # the window was decoded in a several-row session: encode it for the pass
        encoded = _rows_of(model).get(1)
        alignment = T.find_alignment(encoded, tokenizer, text_tokens, mel_segment, num_frames)
    else:                                         # the 1-row session still holds this window's encoder output
        stacker = _align_stacker(model) if text_tokens else None
        if stacker is not None and stacker.group.fits(len(tokenizer.sot_sequence) + 2 + len(text_tokens), num_frames):
            alignment = stacker.align(encoded, tokenizer, text_tokens, num_frames)      # beside the other calls' windows
        else:
            alignment = T.find_alignment(encoded, tokenizer, text_tokens, None, num_frames)
    T.attach_words(segments, alignment, per_segment, last_speech_timestamp=last_speech_timestamp,
                   prepend_punctuations=prepend, append_punctuations=append)


def transcribe_many(model: HipWhisperModel, audios: Sequence, *, stack: int = 8, burst: Optional[int] = None,
                    **kwargs) -> List[dict]:
    """Offline convenience: one :func:`transcribe` per recording on worker threads (at most ``stack`` at a time) whose
    greedy temperature-0 windows share the model's :class:`WindowStacker`; -> the result dictionaries, in order.  The
    model's stack setting is switched to ``stack`` rows - and, when ``burst`` is given, its steps per library call to
    ``burst`` - for the duration of the call and put back afterwards."""
    rows = resolve_stack(stack)
    if rows < 1:
        raise ValueError("transcribe_many needs stack in 1..8")
    audios = list(audios)
    results: List[Optional[dict]] = [None] * len(audios)
    errors: List[Optional[BaseException]] = [None] * len(audios)
    gate = threading.Semaphore(rows)
    before = model.__dict__.get("_window_stack_rows")
    burst_before = model.__dict__.get("_window_stack_burst")
    if burst is not None:
        set_burst(model, burst)
    set_stack(model, rows)

    def work(i: int) -> None:
        with gate:
            try:
                results[i] = transcribe(model, audios[i], **kwargs)
            except BaseException as e:
                errors[i] = e

    threads = [threading.Thread(target=work, args=(i,), name=f"wlk-transcribe-{i}") for i in range(len(audios))]
    try:
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    finally:
        with _STACK_LOCK:
            if before is None:
                model.__dict__.pop("_window_stack_rows", None)
            else:
                model.__dict__["_window_stack_rows"] = before
            if burst is not None:
                if burst_before is None:
                    model.__dict__.pop("_window_stack_burst", None)
                else:
                    model.__dict__["_window_stack_burst"] = burst_before
    for e in errors:
        if e is not None:
            raise e
    return results
