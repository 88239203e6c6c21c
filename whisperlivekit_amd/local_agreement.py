"""LocalAgreement's batch ASR wrapper on the HIP library: the role of ``WhisperASR`` (whisperlivekit/local_agreement/
backends.py:39-98) under the reference's ``OnlineASRProcessor`` (local_agreement/online_asr.py:94-427), which calls
``transcribe(audio_buffer, init_prompt=...)``, ``ts_words(result)``, ``segments_end_ts(result)`` and reads ``sep``.

The policy (HypothesisBuffer, buffer trimming) is host logic of the reference and is not restated here: this object plugs
into it.  ``transcribe`` is :func:`whisperlivekit_amd.transcribe.transcribe` with the arguments the reference wrapper
passes (language, ``initial_prompt``, ``condition_on_previous_text=True``, ``word_timestamps=True`` and the user's
``transcribe_kargs`` minus the VAD switches).  Attributes the reference's ``backend_factory`` sets afterwards
(``tokenizer``, ``confidence_validation``, ``buffer_trimming``, ``buffer_trimming_sec``, ``backend_choice``) are plain
attributes here as well.
"""
from __future__ import annotations

import logging
import sys
from typing import List, Optional

from .backend import load_openai_checkpoint
from .dims import ALIGNMENT_HEADS, MODEL_DIMS
from .engine import HipWhisperModel
from .policy import ASRToken
from .transcribe import (WindowDraft, resolve_align_stack, resolve_burst, resolve_draft, resolve_stack, set_align_stack,
                         set_burst, set_stack, transcribe as hip_transcribe)

logger = logging.getLogger(__name__)


class HipWhisperASR:
    sep = " "         # words of `transcribe` are joined with a space (backends.py:16-17, 41)

    def __init__(self, lan: str, model_size: Optional[str] = None, cache_dir: Optional[str] = None,
                 model_dir: Optional[str] = None, lora_path: Optional[str] = None, logfile=sys.stderr, *, device: int = 0,
                 hip_model: Optional[HipWhisperModel] = None, state_dict=None, synthetic_seed: Optional[int] = None,
                 stack: Optional[int] = None, align_stack: Optional[bool] = None, burst: Optional[int] = None,
                 draft: Optional[bool] = None):
        """``stack``: rows of the model's window group - the greedy temperature-0 steps of up to that many concurrent
        ``transcribe`` calls share each pass over the decoder weights (transcribe.WindowStacker; 0 = off, None = the
        environment's ``WLK_TRANSCRIBE_STACK``, default off).  ``align_stack``: the word-timestamp alignment of those
        calls' windows shares one stacked pass as well (transcribe.AlignStacker; needs ``stack`` >= 1; None = the
        environment's ``WLK_TRANSCRIBE_ALIGN_STACK``, default off).  ``burst``: steps of the window group per library call
        (transcribe.WindowStacker(burst=...), 1..16; needs ``stack`` >= 1; None = the environment's
        ``WLK_TRANSCRIBE_STACK_BURST``, default 1 = one step per call).  ``draft``: a session's ``transcribe`` calls on
        its growing buffer verify the previous call's hypothesis in one decoder pass instead of decoding it again token by
        token (transcribe.WindowDraft; needs ``stack`` >= 1; None = the environment's ``WLK_TRANSCRIBE_DRAFT``,
        default off).  The memory is per session: it lives in :meth:`session_view`, never in this shared object."""
        self.logfile = logfile
        self.transcribe_kargs = {}
        self.lora_path = lora_path
        self.original_language = None if lan == "auto" else lan
        self.tokenizer = None
        self.confidence_validation = False
        self.buffer_trimming = "segment"
        self.buffer_trimming_sec = 15
        self.backend_choice = "whisper"
        if lora_path is not None and model_dir is None:
            raise ValueError("lora_path needs model_dir: the adapter is merged into the checkpoint's weights at load time "
                             "(whisper/__init__.py:337-391)")
        if hip_model is not None:
            self.model = hip_model
        else:
            self.model = self.load_model(model_size, cache_dir, model_dir, device=device, state_dict=state_dict,
                                         synthetic_seed=synthetic_seed)
        self.stack = resolve_stack(stack)
        if stack is not None:
            set_stack(self.model, self.stack)       # an explicit argument wins over the environment
        self.align_stack = resolve_align_stack(align_stack)
        if align_stack is not None:
            if self.align_stack and self.stack < 1:
                raise ValueError("align_stack needs stack >= 1: the stacked alignment runs on the window group")
            set_align_stack(self.model, self.align_stack)
        self.align_stack = self.align_stack and self.stack >= 1
        self.burst = resolve_burst(burst)
        if burst is not None:
            if self.burst > 1 and self.stack < 1:
                raise ValueError("burst needs stack >= 1: the steps per call are the window group's")
            set_burst(self.model, self.burst)       # an explicit argument wins over the environment
        self.draft = resolve_draft(draft)
        if draft is not None and self.draft and self.stack < 1:
            raise ValueError("draft needs stack >= 1: the verify pass runs on the window group")
        self.draft = self.draft and self.stack >= 1

    def load_model(self, model_size=None, cache_dir=None, model_dir=None, *, device: int = 0, state_dict=None,
                   synthetic_seed: Optional[int] = None) -> HipWhisperModel:
        """A local checkpoint in any layout the reference's load_model takes (``model_dir`` = file or directory,
        backends.py:44-61; openai / HuggingFace / MLX names, safetensors, shards, a LoRA adapter merged in:
        checkpoint.load_whisper_checkpoint), a state_dict for a named size, or seeded random weights of a named size (parity /
        timing runs: there is no checkpoint where this is built)."""
        if model_dir is not None:
            from .checkpoint import load_whisper_checkpoint
            dims, sd, own_heads = load_whisper_checkpoint(str(model_dir), self.lora_path)
            return HipWhisperModel.from_state_dict(dims, sd, own_heads or ALIGNMENT_HEADS.get(model_size), device)
        if model_size is None:
            raise ValueError("Either model_size or model_dir must be set for HipWhisperASR")
        if state_dict is not None:
            return HipWhisperModel.from_state_dict(MODEL_DIMS[model_size], state_dict, ALIGNMENT_HEADS.get(model_size), device)
        if synthetic_seed is not None:
            return HipWhisperModel.synthetic(model_size, synthetic_seed, device)
        raise ValueError("no weights: give model_dir (a .pt checkpoint), state_dict or synthetic_seed")

    def transcribe(self, audio, init_prompt: str = "") -> dict:
        return self._transcribe(audio, init_prompt, None)

    def _transcribe(self, audio, init_prompt: str, draft: Optional[WindowDraft]) -> dict:
        options = dict(self.transcribe_kargs)
        options.pop("vad", None)
        options.pop("vad_filter", None)
        if draft is not None:
            options["draft"] = draft
        return hip_transcribe(self.model, audio, language=self.original_language or None, initial_prompt=init_prompt,
                              condition_on_previous_text=True, word_timestamps=True, **options)

    def session_view(self) -> "HipWhisperASRView":
        """The per-session face of this shared object: ``OnlineASRProcessor(asr.session_view())``.  Same duck type, same
        model; with ``draft`` on it owns the one :class:`transcribe.WindowDraft` of its session."""
        return HipWhisperASRView(self)

    def ts_words(self, result: dict) -> List[ASRToken]:
        return [ASRToken(w["start"], w["end"], w["word"], probability=w.get("probability"))
                for segment in result["segments"] for w in segment["words"]]

    def segments_end_ts(self, result: dict) -> List[float]:
        return [segment["end"] for segment in result["segments"]]

    def use_vad(self):
        logger.warning("VAD is not currently supported for the Whisper backend and will be ignored.")


class HipWhisperASRView:
    """What one session hands to the reference's ``OnlineASRProcessor`` in place of the shared :class:`HipWhisperASR`:
    ``transcribe`` / ``ts_words`` / ``segments_end_ts`` / ``sep`` and every attribute ``backend_factory`` sets are the shared
    object's (read and written through), the draft memory is this view's own."""
    _OWN = ("asr", "memory")

    def __init__(self, asr: HipWhisperASR):
        object.__setattr__(self, "asr", asr)
        object.__setattr__(self, "memory", WindowDraft() if asr.draft else None)

    def __getattr__(self, name):                   # only reached for names this view does not own
        return getattr(self.asr, name)

    def __setattr__(self, name, value):
        if name in self._OWN:
            object.__setattr__(self, name, value)
        else:
            setattr(self.asr, name, value)

    def transcribe(self, audio, init_prompt: str = "") -> dict:
        return self.asr._transcribe(audio, init_prompt, self.memory)
