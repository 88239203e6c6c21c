"""Config 5 session glue: the per-session translation object ``AudioProcessor.translation_processor`` drives
(whisperlivekit/audio_processor.py:887-920), over the NLLB / M2M-100 network of :mod:`whisperlivekit_amd.nllb`.

What the reference does: ``TranscriptionEngine`` loads ONE shared model through the third-party ``nllw`` package
(``core.py:320-329``: ``nllw.load_model([source], nllb_backend=, nllb_size=)``) and every session gets its own
``nllw.OnlineTranslation(model, [source], [target])`` (``core.py:483-493``; per-session target languages:
``translation.py:17-47``).  ``nllw`` is NOT in the reference tree and no test there pins its numerics or its policy.
What IS in the tree is the contract those objects must meet - the four calls at ``audio_processor.py:903-911`` - and a
second implementation of that contract, ``AlignAttTranslationClient`` (``translation_alignatt.py:99-181``, "duck-typed
contract (mirrors nllw.OnlineTranslation)"):

* ``insert_tokens(items)``: the ASR's newly committed ``ASRToken`` s (``HypothesisTail`` items only for backends that
  ask for them with ``wants_hypothesis_tail`` - this one does not);
* ``process() -> (Translation | None, TimedText)``: newly VALIDATED target text (appended to ``state.new_translation``,
  append-only on screen) and the current unstable buffer (replaces ``state.new_translation_buffer``);
* ``validate_buffer_and_reset() -> (Translation, TimedText)``: at a silence start / speaker change the open buffer is
  validated as it stands and the session starts a fresh segment;
* ``insert_silence(duration)``.

The policy between those calls (WHEN to re-translate WHICH source prefix, and how much of a hypothesis to validate) is
``nllw``'s own and is restated here FROM THE CALL CONTRACT ONLY, as the standard local-agreement rule of simultaneous
translation (the rule the reference itself uses for ASR hypotheses, ``local_agreement/online_asr.py``): the open source
segment (committed words since the last sentence end) is re-translated whenever it grew; target words on which two
successive hypotheses agree are validated, the rest of the newest hypothesis is the buffer; a source word that carries
sentence punctuation (``TimedText.has_punctuation``, timed_objects.py:28-29) closes the segment - its final translation
is validated whole and the next segment starts with an empty history.  Timestamps are the source words': a validated
piece spans from where the last one ended to the end of the newest source word it was produced from.

Device work per ``process()``: one encoder pass over the open segment and one greedy (or beam) decode -
``nllb.generate`` / ``nllb.beam_search`` with ``forced_bos_token_id`` = the target language code, exactly the calls
``transformers``' NLLB recipe makes.  Tokenisation is the caller's: any object with the ``transformers`` tokenizer
surface this module uses (``src_lang`` attribute, ``__call__(text).input_ids``, ``convert_tokens_to_ids(lang)``,
``decode(ids, skip_special_tokens=True)``) - ``transformers.NllbTokenizer`` over the checkpoint's
``sentencepiece.bpe.model`` in deployment, a seeded stand-in in the tests (no SentencePiece model exists offline).
No CPU fallback: the model is a :class:`whisperlivekit_amd.nllb.HipNllbModel`.

Opt-in AlignAtt policy (``HipNllbTranslationModel(policy="alignatt")``): :class:`HipAlignAttTranslation`
meets the same four calls with the policy config 5 names.  The decoder's own cross-attention says which source token a
target token was produced from; a token that leans on the newest, still unstable source words is held back and everything
before it is committed at once; the next update decodes on from the committed target ids, so the text on screen only
grows.  The reference reaches this policy through a WebSocket client of an external sidecar
(``translation_alignatt.py:99-181``); what is restated here is that client's observable contract, not its wire protocol.

Opt-in stacking (``HipNllbTranslationModel(stack=n)`` / ``WLK_NLLB_STACK=n``, greedy decoding only): the model owns ONE
``HipNllbBatch`` of n slots and every session hands the segments of a ``process()`` - the closed sentences and the open
one - to it as one request list; sentences of different sessions that are in flight at the same time share every decoder
weight pass (``nllb.generate_batch``).  The validated text and the buffers are the ones of the default path.

Stacked AlignAtt (``policy="alignatt", stack=n``): the batch has the alignment heads set, and every
update or final pass of every session is ONE request to :class:`NllbAlignAttStacker` - updates of different sessions that
fall on the same ASR tick share the stacked encode, the stacked prefill of their committed ids and every decoder step
(``nllb.generate_alignatt_batch``).  The sessions hold no device state; their texts are those of the unstacked policy.
"""
from __future__ import annotations

import logging
import os
import threading
import time
from dataclasses import dataclass, field
from typing import Any, Callable, List, Optional, Sequence, Tuple

from . import nllb

logger = logging.getLogger(__name__)

PUNCTUATION_MARKS = {".", "!", "?", "。", "！", "？"}        # timed_objects.py:4


@dataclass
class TimedText:
    """whisperlivekit/timed_objects.py:19-44 (the fields the translation path reads / writes)."""
    start: Optional[float] = 0
    end: Optional[float] = 0
    text: Optional[str] = ""
    speaker: Optional[int] = -1
    detected_language: Optional[str] = None

    def has_punctuation(self) -> bool:
        return any(ch in PUNCTUATION_MARKS for ch in (self.text or "").strip())

    def __bool__(self) -> bool:
        return bool(self.text)


@dataclass
class Translation(TimedText):
    """timed_objects.py:96-97"""


def _has_punctuation(item: Any) -> bool:
    fn = getattr(item, "has_punctuation", None)
    if callable(fn):
        return bool(fn())
    return any(ch in PUNCTUATION_MARKS for ch in (getattr(item, "text", "") or "").strip())


def _common_prefix(a: Sequence[str], b: Sequence[str]) -> int:
    n = 0
    for x, y in zip(a, b):
        if x != y:
            break
        n += 1
    return n


def resolve_draft(draft: Optional[bool]) -> bool:
    """``HipNllbTranslationModel(draft=...)``: an explicit value wins; ``None`` reads ``WLK_NLLB_DRAFT`` (default off)."""
    if draft is None:
        return os.environ.get("WLK_NLLB_DRAFT", "0").strip() == "1"
    return bool(draft)


def resolve_stack(stack: Optional[int]) -> int:
    """``HipNllbTranslationModel(stack=...)``: an explicit value wins; ``None`` reads ``WLK_NLLB_STACK`` (default 0 = off)."""
    if stack is None:
        stack = int(os.environ.get("WLK_NLLB_STACK", "0").strip() or 0)
    stack = int(stack)
    if stack < 0 or stack > 8:
        raise ValueError("stack must be 0 (off) or 1..8 slots")
    return stack


class NllbStacker:
    """Thread-safe front of one ``HipNllbBatch``: any session thread calls :meth:`translate_many`; the first caller becomes
    the runner and drives ``nllb.generate_batch``, callers that arrive while a pass is running queue their requests - the
    runner's ``more`` callback admits them at its next step - and wait on a condition for their tickets.  The runner keeps
    running until the batch is empty and nobody is queued.  A pass that fails hands its error to every request in flight
    or queued, so no waiter blocks for ever; the slots are released and the next caller starts a fresh pass."""

    def __init__(self, batch: Any):
        self.batch = batch
        self._cv = threading.Condition()
        self._queue: List[tuple] = []              # (source, forced_bos, max_new_tokens, ticket) not yet handed to the pass
        self._open: set = set()                    # tickets queued or in flight
        self._outcome: dict = {}                   # ticket -> (ids, error)
        self._running = False
        self._next_ticket = 0
        self.passes = 0                            # generate_batch passes run (bench / tests)
        self.sentences = 0

    def translate_many(self, requests: Sequence[tuple]) -> List[List[int]]:
        """``requests``: ``(source ids, forced_bos_token_id, max_new_tokens)`` per sentence -> their ids, in order.  A request
        may carry a fourth element, the draft ``nllb.generate_batch`` verifies (a previous result of the sentence, or ``None``)."""
        return self._submit([(list(req[0]), req[1], int(req[2]), *req[3:4]) for req in requests])

    def _drive(self, more, done) -> None:
        """one pass over the batch: returns when the batch is empty and ``more`` has nothing left"""
        def more_in_order():                       # the queue keeps the ticket last; generate_batch takes the draft behind it
            return [it if len(it) == 4 else (it[0], it[1], it[2], it[4], it[3]) for it in (more() or ())]

        nllb.generate_batch(self.batch, [], more=more_in_order, done=done)

    def _submit(self, requests: Sequence[tuple]) -> list:
        """queues ``requests`` (the pass's request tuples, without ticket) and waits for their outcomes, driving the pass if
        nobody else is"""
        if not requests:
            return []
        with self._cv:
            tickets = list(range(self._next_ticket, self._next_ticket + len(requests)))
            self._next_ticket += len(requests)
            for t, req in zip(tickets, requests):
                self._queue.append((*req, t))
                self._open.add(t)
        while True:
            with self._cv:
                while self._running and any(t not in self._outcome for t in tickets):
                    self._cv.wait()
                if all(t in self._outcome for t in tickets):
                    got = [self._outcome.pop(t) for t in tickets]
                    for _ids, err in got:
                        if err is not None:
                            raise err
                    return [ids for ids, _err in got]
                self._running = True               # nobody is driving the batch and this caller still waits: it drives
            self._run()

    def _run(self) -> None:
        def more():
            with self._cv:
                items, self._queue = self._queue, []
            return items

        def done(ticket, ids):
            with self._cv:
                self._outcome[ticket] = (ids, None)
                self._open.discard(ticket)
                self.sentences += 1
                self._cv.notify_all()

        error: Optional[BaseException] = None
        try:
            self._drive(more, done)
        except BaseException as e:                 # the pass is gone: everyone in it or queued behind it gets the error
            error = e
            for slot in range(self.batch.n_slots):  # the next pass starts from free slots
                try:
                    self.batch.release(slot)
                except Exception:                   # the callers receive the pass's own error
                    pass
        finally:
            with self._cv:
                self.passes += 1
                if error is not None:
                    for t in self._open:
                        self._outcome[t] = (None, error)
                    self._open.clear()
                    self._queue = []
                self._running = False
                self._cv.notify_all()
        if error is not None and not isinstance(error, Exception):
            raise error


class NllbAlignAttStacker(NllbStacker):
    """:class:`NllbStacker` for ``policy="alignatt"``: the same queue, runner and failure contract over
    ``nllb.generate_alignatt_batch``; ``passes`` counts its passes, ``sentences`` the updates and finals they served."""

    def decode_many(self, requests: Sequence[tuple]) -> List[Tuple[List[int], List[int], str]]:
        """``requests``: ``(source ids, forced_bos_token_id, committed ids, n_accessible, threshold, final, max_new_tokens)`` per
        update -> ``(new ids, their source positions, stop reason)`` each, in order."""
        return self._submit([(list(src), int(bos), [int(t) for t in committed], int(n_acc), int(thr), bool(final), int(max_new))
                             for src, bos, committed, n_acc, thr, final, max_new in requests])

    def _drive(self, more, done) -> None:
        nllb.generate_alignatt_batch(self.batch, [], more=more, done=done)


class HipNllbTranslationModel:
    """The server-wide handle ``nllw.load_model`` returns in the reference (``TranscriptionEngine.translation_model``,
    core.py:320-329): one network per GPU shared by every session, plus the tokenizer and the decoding options.  Device
    sessions are 1-row and cheap; each ``HipOnlineTranslation`` owns one, so sessions never share decoder caches.
    ``num_beams`` > 1 gives every session that many rows and ``nllb.beam_search``; ``WLK_NLLB_BEAM_STEPS=1`` in the
    environment moves its steps onto the device (``step_beam``; off by default)."""

    def __init__(self, model: nllb.HipNllbModel, tokenizer: Any, num_beams: int = 1, max_new_tokens: int = 199,
                 max_source_tokens: int = 200, stack: Optional[int] = None, policy: str = "local_agreement", threshold: int = 2,
                 alignment_heads: Optional[Sequence[Tuple[int, int]]] = None, hypothesis_tail: bool = False,
                 draft: Optional[bool] = None):
        """``policy="alignatt"`` (opt-in, greedy only): sessions are :class:`HipAlignAttTranslation`; a target token whose
        source position lies within ``threshold`` tokens of the end of the committed source is held back;
        ``alignment_heads`` = ``(decoder layer, head)`` pairs, ``None`` = ``nllb.default_alignment_heads`` - neither that
        default nor ``threshold=2`` has been validated on trained weights; ``hypothesis_tail`` asks the ASR for its unstable
        tail and feeds it to the encoder as context no token may be committed from.

        ``policy="alignatt"`` with ``stack=n`` (or ``WLK_NLLB_STACK=n``) stacks: the model owns one batch of n slots with
        the alignment heads set and a :class:`NllbAlignAttStacker`, and the sessions submit their updates to it instead of
        owning a device session.  (Before DESIGN.md section 22 this combination silently ran unstacked.)

        ``draft`` (opt-in; ``None`` reads ``WLK_NLLB_DRAFT``, default off): every session hands the
        ids of the open sentence's previous hypothesis to its next update as a draft, verified in one stacked decoder pass.
        Needs ``stack >= 1``, ``num_beams == 1`` and ``policy="local_agreement"`` (``ValueError`` otherwise); the texts are
        those of ``draft=False``."""
        if policy not in ("local_agreement", "alignatt"):
            raise ValueError("policy must be 'local_agreement' or 'alignatt'")
        if policy == "alignatt" and int(num_beams) != 1:
            raise ValueError("policy='alignatt' decodes greedily (num_beams = 1)")
        if int(threshold) < 0:
            raise ValueError("threshold must be >= 0")
        self.policy, self.threshold, self.hypothesis_tail = policy, int(threshold), bool(hypothesis_tail)
        self.alignment_heads = None if alignment_heads is None else [(int(l), int(h)) for l, h in alignment_heads]
        self.model, self.tokenizer = model, tokenizer
        self.num_beams, self.max_new_tokens, self.max_source_tokens = int(num_beams), int(max_new_tokens), int(max_source_tokens)
        # a tokenizer with a mutable src_lang (transformers' NllbTokenizer) is shared by all sessions
        self.tokenizer_lock = threading.Lock()
        # opt-in: one batch of `stack` slots shared by every session (greedy decoding only; beams keep their own sessions)
        self.stack = resolve_stack(stack) if self.num_beams == 1 else 0
        self.batch = model.new_batch(self.stack) if self.stack else None
        self.draft = resolve_draft(draft)
        if self.draft and not (self.stack >= 1 and self.num_beams == 1 and policy == "local_agreement"):
            if self.batch is not None:
                self.batch.close()
            raise ValueError("draft verification needs stack >= 1, num_beams = 1 and policy='local_agreement'")
        self.stacker = None
        if self.batch is not None and policy == "alignatt":
            heads = self.alignment_heads if self.alignment_heads is not None else nllb.default_alignment_heads(model.cfg)
            self.batch.set_alignment_heads(heads)
            self.stacker = NllbAlignAttStacker(self.batch)
        elif self.batch is not None:
            self.stacker = NllbStacker(self.batch)

    def language_id(self, code: str) -> int:
        tid = self.tokenizer.convert_tokens_to_ids(code)
        unk = getattr(self.tokenizer, "unk_token_id", None)
        if tid is None or (unk is not None and tid == unk):
            raise ValueError(f"unknown NLLB language code {code!r}")          # translation.py:40-46 catches ValueError
        return int(tid)

    def encode(self, text: str, src_lang: str) -> List[int]:
        with self.tokenizer_lock:
            self.tokenizer.src_lang = src_lang
            ids = list(self.tokenizer(text).input_ids)
        if len(ids) > self.max_source_tokens:                 # keep the language code (first) and </s> (last)
            ids = ids[:1] + ids[-(self.max_source_tokens - 1):]
        return ids

    def decode(self, ids: Sequence[int]) -> str:
        return self.tokenizer.decode(list(ids), skip_special_tokens=True)

    def new_session(self, source_language: str, target_language: str):
        return _session_class(self)(self, [source_language], [target_language])

    def close(self) -> None:
        """Releases the shared batch (the network itself belongs to the caller)."""
        batch, self.batch, self.stacker = self.batch, None, None
        if batch is not None:
            batch.close()


@dataclass
class _Segment:
    tokens: List[Any] = field(default_factory=list)          # source words (ASRToken-like) of the open sentence

    @property
    def start(self) -> Optional[float]:
        return self.tokens[0].start if self.tokens else None

    @property
    def end(self) -> Optional[float]:
        return self.tokens[-1].end if self.tokens else None

    def text(self) -> str:
        # ASR words carry their own leading spaces (simul_whisper) or not (LocalAgreement: asr.sep): normalise
        return " ".join((t.text or "").strip() for t in self.tokens if (t.text or "").strip())


class HipOnlineTranslation:
    """``nllw.OnlineTranslation(model, [source], [target])`` for one session (constructed at core.py:490-493 /
    translation.py:36-39); duck type of audio_processor.py:903-911.  One call in flight per session
    (``translation_processor`` awaits ``to_thread(self.translation.process)``); different sessions run concurrently on
    their own device sessions."""

    wants_hypothesis_tail = False          # audio_processor.py only queues HypothesisTail items to backends that ask

    def __init__(self, translation_model: HipNllbTranslationModel, source_languages: Sequence[str],
                 target_languages: Sequence[str]):
        if not source_languages or not target_languages:
            raise ValueError("source and target language lists must not be empty")
        self.shared = translation_model
        self.source_language, self.target_language = source_languages[0], target_languages[0]
        self.target_id = translation_model.language_id(self.target_language)       # ValueError for an unknown code
        translation_model.language_id(self.source_language)
        # stacked serving: the sentences live in the slots of the model's batch, the session needs no device state of its own
        self.session = (translation_model.model.new_session(rows=max(1, translation_model.num_beams))
                        if translation_model.stacker is None else None)
        self._ready: List[List[str]] = []          # stacked serving: this call's hypotheses, in the order process() asks for them
        self._segment = _Segment()
        self._closed: List[_Segment] = []          # sentences that ended (punctuation) and await their final translation
        self._validated_words: List[str] = []      # target words of the open segment already handed out
        self._previous: List[str] = []             # previous hypothesis of the open segment (target words)
        self._previous_ids: Optional[List[int]] = None   # ... and its ids, the next update's draft (draft serving only)
        self._hyp_ids: Optional[List[int]] = None  # draft serving: the ids of this call's hypothesis of the open segment
        self._buffer_words: List[str] = []
        self._dirty = False
        self._last_end: Optional[float] = None     # end time of the last validated piece
        self._silence = 0.0
        self.translations = 0                      # device translations run (bench / tests)

    # ---- duck type --------------------------------------------------------------------------------------------------
    def insert_tokens(self, items: List[Any]) -> None:
        for item in items:
            if type(item).__name__ == "HypothesisTail" or not hasattr(item, "text") or not hasattr(item, "end"):
                continue
            if not (item.text or "").strip():
                continue
            self._segment.tokens.append(item)
            self._dirty = True
            if _has_punctuation(item):
                self._closed.append(self._segment)
                self._segment = _Segment()

    def process(self) -> Tuple[Optional[Translation], TimedText]:
        if self.shared.stacker is not None:           # every segment this call translates, as ONE request list
            self._ready = self._translate_many(self._closed + ([self._segment] if self._segment.tokens and self._dirty else []))
        pieces: List[str] = []
        end: Optional[float] = None
        start = self._piece_start(self._closed[0].start if self._closed else self._segment.start)
        for seg in self._closed:                      # finished sentences: their last translation is final
            words = self._translate(seg)
            # validated text is append-only: only what lies behind it is new.  "Behind it" is by CONTENT, not by count - a
            # final hypothesis that rewrote or shortened the validated prefix continues from where the two still agree, so no
            # word is dropped or printed twice (the open-sentence path below makes the same check)
            keep = _common_prefix(words, self._validated_words)
            if keep != len(self._validated_words):
                logger.debug("final translation rewrites %d validated word(s)", len(self._validated_words) - keep)
            pieces += words[keep:]
            end = seg.end
            self._validated_words, self._previous, self._buffer_words = [], [], []
            self._previous_ids = None
        self._closed = []
        if self._segment.tokens and self._dirty:      # the open sentence: local agreement of two successive hypotheses
            hyp = self._translate(self._segment)
            agreed = _common_prefix(hyp, self._previous)
            n_val = len(self._validated_words)
            if hyp[:n_val] != self._validated_words:
                # the new hypothesis rewrites validated text: on screen that text is append-only, so it stays; nothing
                # new is validated until the hypotheses settle behind it
                agreed = 0
            if agreed > n_val:
                pieces += hyp[n_val:agreed]
                self._validated_words = hyp[:agreed]
                end = self._segment.end
            self._previous = hyp
            self._previous_ids = self._hyp_ids
            self._buffer_words = hyp[len(self._validated_words):] if hyp[:len(self._validated_words)] == self._validated_words else []
        self._dirty = False
        new = None
        if pieces:
            new = Translation(start=start, end=end if end is not None else start, text=" ".join(pieces))
            self._last_end = new.end
        return new, self._buffer()

    def validate_buffer_and_reset(self) -> Tuple[Translation, TimedText]:
        """Silence start / speaker change (audio_processor.py:903-908): what is on screen as the buffer becomes validated
        text, pending sentences are translated now, and the next words start a fresh segment."""
        pending, buffer_words = None, list(self._buffer_words)
        if self._closed or (self._segment.tokens and self._dirty):
            pending, _ = self.process()
            buffer_words = list(self._buffer_words)
        start = self._piece_start(self._segment.start)
        text = " ".join(([pending.text] if pending else []) + buffer_words)
        end = self._segment.end if (buffer_words and self._segment.end is not None) else (pending.end if pending else start)
        validated = Translation(start=pending.start if pending else start, end=end, text=text)
        if validated.text:
            self._last_end = validated.end
        self._segment = _Segment()
        self._validated_words, self._previous, self._buffer_words = [], [], []
        self._previous_ids = None
        self._dirty = False
        return validated, TimedText()

    def insert_silence(self, duration: Optional[float]) -> None:
        """audio_processor.py:909-911: the ASR tokens that follow already carry the shifted times; kept for the record."""
        self._silence += float(duration or 0.0)

    def close(self) -> None:
        if self.session is not None:
            self.session.close()

    # ---- internals --------------------------------------------------------------------------------------------------
    def _piece_start(self, fallback: Optional[float]) -> float:
        if self._last_end is not None:
            return self._last_end
        return fallback if fallback is not None else 0.0

    def _buffer(self) -> TimedText:
        if not self._buffer_words:
            return TimedText()
        return TimedText(start=self._piece_start(self._segment.start), end=self._segment.end, text=" ".join(self._buffer_words))

    def _translate_many(self, segs: Sequence[_Segment]) -> List[List[str]]:
        m = self.shared
        requests = [(m.encode(seg.text(), self.source_language), self.target_id, m.max_new_tokens) for seg in segs]
        if getattr(m, "draft", False) and segs:
            # the open sentence's last hypothesis is the draft of whatever continues that sentence: its next update (the
            # open segment itself) or, when punctuation closed it, its final translation (the first closed segment)
            requests[0] = (*requests[0], self._previous_ids)
        outs = m.stacker.translate_many(requests)
        self.translations += len(outs)
        self._hyp_ids = list(outs[-1]) if getattr(m, "draft", False) and segs and segs[-1] is self._segment else None
        return [m.decode(out).split() for out in outs]

    def _translate(self, seg: _Segment) -> List[str]:
        if self._ready:                               # stacked serving: translated at the top of process()
            return self._ready.pop(0)
        m = self.shared
        src = m.encode(seg.text(), self.source_language)
        if m.num_beams > 1:
            out = nllb.beam_search(self.session, src, self.target_id, num_beams=m.num_beams, max_new_tokens=m.max_new_tokens)
        else:
            out = nllb.generate(self.session, src, self.target_id, max_new_tokens=m.max_new_tokens)
        self.translations += 1
        return m.decode(out).split()


@dataclass
class _Sentence:
    """One source sentence under the AlignAtt policy: its committed source words and the target ids committed so far."""
    segment: _Segment = field(default_factory=_Segment)
    ids: List[int] = field(default_factory=list)      # committed target ids (append-only)
    text: str = ""                                    # their decoded text as it stands on screen
    validated: int = 0                                # characters of `text` already handed out as validated


class HipAlignAttTranslation:
    """The AlignAtt session object (``policy="alignatt"``): duck type of audio_processor.py:903-911, with the observable
    contract of the reference's sidecar client (translation_alignatt.py:99-181; selected at core.py:305-318, 483-493):

    * per open sentence a list of committed target ids; ``process()`` on it runs ONE non-final
      ``nllb.generate_alignatt`` from those ids, appends what that emitted and returns ``(None, TimedText(text))`` - the
      text on screen is replaced only by a text that starts with it;
    * a source word with sentence punctuation ends the sentence: ``process()`` runs one FINAL pass from its committed ids
      and returns the whole sentence as one ``Translation`` from the last segment's end to the sentence's end - one
      finished sentence per call, the rest on the next calls;
    * ``validate_buffer_and_reset()`` returns the text on screen as validated, queues the sentence for its final pass
      (which then hands out only what lies behind the validated text) and starts a fresh segment;
    * ``hypothesis_tail``: the newest ``HypothesisTail`` text is appended to the source as words no token may be committed
      from; a change of the tail alone re-runs the update at most every ``TAIL_INTERVAL`` seconds.

    One call in flight per session; the device session is 1-row.  Over a stacked model (``stack=n``) there is no device
    session: every update and final is one request to the model's :class:`NllbAlignAttStacker`."""

    TAIL_INTERVAL = 0.5

    def __init__(self, translation_model: HipNllbTranslationModel, source_languages: Sequence[str],
                 target_languages: Sequence[str], clock: Callable[[], float] = time.monotonic):
        if not source_languages or not target_languages:
            raise ValueError("source and target language lists must not be empty")
        self.shared = translation_model
        self.source_language, self.target_language = source_languages[0], target_languages[0]
        self.target_id = translation_model.language_id(self.target_language)       # ValueError for an unknown code
        translation_model.language_id(self.source_language)
        self.wants_hypothesis_tail = bool(translation_model.hypothesis_tail)
        self.session = None
        if translation_model.stacker is None:
            self.session = translation_model.model.new_session(rows=1)
            heads = translation_model.alignment_heads
            self.session.set_alignment_heads(heads if heads is not None else nllb.default_alignment_heads(translation_model.model.cfg))
        self._device_loop = hasattr(self.session, "generate_alignatt_loop")
        self._clock = clock
        self._open = _Sentence()
        self._finals: List[_Sentence] = []         # ended sentences awaiting their final pass, oldest first
        self._tail = ""
        self._dirty = False                        # committed words arrived since the last update
        self._tail_dirty = False
        self._last_run: Optional[float] = None
        self._last_end: Optional[float] = None
        self._silence = 0.0
        self.updates = self.finals = 0             # device passes run (bench / tests)
        self.last_n_accessible: Optional[int] = None

    # ---- duck type --------------------------------------------------------------------------------------------------
    def insert_tokens(self, items: List[Any]) -> None:
        for item in items:
            if type(item).__name__ == "HypothesisTail":
                text = " ".join((getattr(item, "text", "") or "").split())
                if self.wants_hypothesis_tail and text != self._tail:
                    self._tail, self._tail_dirty = text, True
                continue
            if not hasattr(item, "text") or not hasattr(item, "end") or not (item.text or "").strip():
                continue
            self._open.segment.tokens.append(item)
            self._dirty = True
            if _has_punctuation(item):
                self._finals.append(self._open)
                self._open = _Sentence()
                self._tail, self._tail_dirty, self._dirty = "", False, False

    def process(self) -> Tuple[Optional[Translation], TimedText]:
        while self._finals:                           # one finished sentence per call
            sent = self._finals.pop(0)
            src = self.shared.encode(sent.segment.text(), self.source_language)
            self._decode_on(sent, src, len(src), final=True)
            self.finals += 1
            piece = sent.text[sent.validated:].strip()         # (behind what a reset already handed out)
            if piece:
                new = Translation(start=self._piece_start(sent.segment.start), end=sent.segment.end, text=piece)
                self._last_end = new.end
                return new, self._buffer()
        sent = self._open
        if not sent.segment.tokens and not self._tail:
            return None, self._buffer()
        now = self._clock()
        if not self._dirty and not (self._tail_dirty and (self._last_run is None or now - self._last_run >= self.TAIL_INTERVAL)):
            return None, self._buffer()
        committed_text = sent.segment.text()
        src_committed = self.shared.encode(committed_text, self.source_language)
        src = self.shared.encode((committed_text + " " + self._tail).strip(), self.source_language) if self._tail else src_committed
        # source positions that belong to committed words: what the two encodings share in front of the committed one's
        # </s> - a tokenizer that merges the last committed word with the tail can only make this smaller
        n_accessible = _common_prefix(src_committed[:-1], src)
        self.last_n_accessible = n_accessible
        self._dirty = self._tail_dirty = False
        self._last_run = now
        if n_accessible - self.shared.threshold > 1:  # else the limit is the window's start and no token can be committed
            self._decode_on(sent, src, n_accessible, final=False)
            self.updates += 1
        return None, self._buffer()

    def validate_buffer_and_reset(self) -> Tuple[Translation, TimedText]:
        """Silence start / speaker change: what is on screen becomes validated as it stands (shown text is never taken
        back), its sentence is queued for a final pass, and the next words start a fresh segment."""
        sent = self._finals[0] if self._finals else self._open
        start = self._piece_start(sent.segment.start)
        text = sent.text[sent.validated:].strip()
        validated = Translation(start=start, end=sent.segment.end if sent.segment.end is not None else start, text=text)
        sent.validated = len(sent.text)
        if self._open.segment.tokens:
            self._finals.append(self._open)
        self._open = _Sentence()
        self._tail, self._tail_dirty, self._dirty = "", False, False
        if validated.text:
            self._last_end = validated.end
        return validated, TimedText()

    def insert_silence(self, duration: Optional[float]) -> None:
        self._silence += float(duration or 0.0)

    def close(self) -> None:
        if self.session is not None:
            self.session.close()

    # ---- internals --------------------------------------------------------------------------------------------------
    def _decode_on(self, sent: _Sentence, src: Sequence[int], n_accessible: int, final: bool) -> None:
        m = self.shared
        room = m.max_new_tokens - len(sent.ids)
        if m.stacker is not None:                     # stacked serving: one request, decoded beside other sessions' updates
            (new_ids, _align, _why), = m.stacker.decode_many([(src, self.target_id, sent.ids, n_accessible, m.threshold, final,
                                                               max(room, 0))])
        else:
            new_ids, _align, _why = nllb.generate_alignatt(self.session, src, self.target_id, committed=sent.ids,
                                                           n_accessible=n_accessible, threshold=m.threshold, final=final,
                                                           max_new_tokens=max(room, 0), device_loop=self._device_loop)
        sent.ids = sent.ids + [int(t) for t in new_ids]
        text = m.decode(sent.ids).strip()
        if text.startswith(sent.text):
            sent.text = text

    def _piece_start(self, fallback: Optional[float]) -> float:
        if self._last_end is not None:
            return self._last_end
        return fallback if fallback is not None else 0.0

    def _buffer(self) -> TimedText:
        sent = self._finals[0] if self._finals else self._open
        text = sent.text[sent.validated:].strip()
        if not text:
            return TimedText()
        return TimedText(start=self._piece_start(sent.segment.start), end=sent.segment.end, text=text)


def _session_class(translation_model: Any):
    return HipAlignAttTranslation if getattr(translation_model, "policy", "local_agreement") == "alignatt" else HipOnlineTranslation


def online_translation_factory(translation_model: HipNllbTranslationModel, source_language: str, target_language: str,
                               fallback_target: Optional[str] = None):
    """core.py:483-493 / translation.py:17-47 for this backend: a session object for ``target_language`` (the model's policy
    decides its class); an unknown per-session target falls back to the server-wide one (``fallback_target``) like
    translation.py:40-47."""
    cls = _session_class(translation_model)
    try:
        return cls(translation_model, [source_language], [target_language])
    except ValueError:
        if fallback_target is None or fallback_target == target_language:
            raise
        return cls(translation_model, [source_language], [fallback_target])
