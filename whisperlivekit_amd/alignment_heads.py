"""Alignment heads for a checkpoint that has no table: a fine-tune, a distilled model, any load by path.

A restatement of the reference's ``scripts/determine_alignment_heads.py`` (docs/default_and_custom_models.md:89) for this
backend, which has no CPU path the script could run on:

  collect_heads (:125-178)   per clip: pad_or_trim to 30 s, log-mel, ONE teacher-forced decoder pass over
                             [sot sequence, <|notimestamps|>, transcript tokens, <|endoftext|>]; per decoder layer and
                             head softmax of the cross-attention scores over the first num_frames // 2 positions, the peak
                             probability of every token row; strength = mean peak, vote = any row more than 3 biased
                             standard deviations (+ 1e-6) above the mean; both averaged over the clips
  selection (:284-287)       strengths > 0.05 (votes > 0.5 is the alternative the script carries commented out)
  the dump (:270-274)        base85(gzip(bool[n_text_layer][n_text_head])): the format of whisper's own tables, what
                             ``--custom-alignment-heads`` carries (whisper/__init__.py:549-551, model.py:363-370)

The pass and the peaks run on the GPU (``HipSession.head_survey``: the scores are never stored - the peak of a softmax row
is 1 / sum exp(s - max s)); mean, deviation and vote are three tiny reductions per head and stay here, in float64.

Command line:  python -m whisperlivekit_amd.alignment_heads --model PATH [--lora PATH] --clips MANIFEST.jsonl
                      [--language en] [--min-strength 0.05] --output alignment_heads.b85
Every manifest line is {"audio": "x.wav" | "x.npy", "text": "..."}: 16 kHz mono WAV or float32 .npy, relative paths
counted from the manifest."""
from __future__ import annotations

import argparse
import base64
import gzip
import json
import logging
import os
import sys
import wave
from typing import Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np

logger = logging.getLogger(__name__)

SAMPLE_RATE = 16000
N_SAMPLES = 30 * SAMPLE_RATE
N_FRAMES = 3000


# ---- the head mask and its dump ----------------------------------------------------------------------------------
def dump_mask(mask) -> str:
    """bool [n_text_layer, n_text_head] -> base85(gzip(bytes)) (determine_alignment_heads.py:270-274)."""
    m = np.ascontiguousarray(np.asarray(mask).astype(np.bool_))
    if m.ndim != 2:
        raise ValueError("dump_mask: expected a [n_text_layer, n_text_head] mask")
    return base64.b85encode(gzip.compress(m.tobytes())).decode("ascii")


def load_mask(text: Union[str, bytes], dims) -> np.ndarray:
    """The dump -> bool [n_text_layer, n_text_head], as Whisper.set_alignment_heads decodes it (whisper/model.py:363-370)."""
    raw = text.strip() if isinstance(text, (bytes, bytearray)) else str(text).strip().encode("ascii")
    flat = np.frombuffer(gzip.decompress(base64.b85decode(raw)), dtype=np.bool_)
    if flat.size != dims.n_text_layer * dims.n_text_head:
        raise ValueError(f"alignment-head dump holds {flat.size} heads, the model has {dims.n_text_layer} x {dims.n_text_head}")
    return flat.reshape(dims.n_text_layer, dims.n_text_head).copy()


def mask_pairs(mask) -> List[Tuple[int, int]]:
    """(layer, head) of every set entry in row-major order - the order of mask.to_sparse().indices()."""
    return [(int(l), int(h)) for l, h in zip(*np.nonzero(np.asarray(mask)))]


def resolve_custom_heads(custom, dims) -> Optional[List[Tuple[int, int]]]:
    """``custom_alignment_heads`` as the backend takes it: None / empty, a sequence of (layer, head) pairs, or the dump
    string that the reference's --custom-alignment-heads carries."""
    if custom is None:
        return None
    if isinstance(custom, (str, bytes, bytearray)):
        return mask_pairs(load_mask(custom, dims))
    pairs = [(int(l), int(h)) for l, h in custom]
    return pairs or None


# ---- one clip ----------------------------------------------------------------------------------------------------
def survey_tokens(tokenizer, transcript: str) -> List[int]:
    """[*sot_sequence, no_timestamps, *encode(transcript), eot] (determine_alignment_heads.py:139-147)."""
    return [*(int(t) for t in tokenizer.sot_sequence), int(tokenizer.no_timestamps),
            *(int(t) for t in tokenizer.encode(transcript)), int(tokenizer.eot)]


def fold_clip(peaks, z_threshold: float = 3.0) -> Tuple[np.ndarray, np.ndarray]:
    """peaks [L, H, P] (float32 from the device) -> (strength [L, H] = mean over the rows, vote [L, H] = any row whose
    z-score - biased deviation + 1e-6 - exceeds the threshold), in float64 (determine_alignment_heads.py:168-174)."""
    p = np.asarray(peaks, np.float64)
    mean = p.mean(axis=-1, keepdims=True)
    z = (p - mean) / (p.std(axis=-1, keepdims=True) + 1e-6)
    return mean[..., 0], (z > z_threshold).any(axis=-1)


def pad_or_trim_audio(audio: np.ndarray, length: int = N_SAMPLES) -> np.ndarray:
    """whisper/audio.py:pad_or_trim of a waveform: cut to 30 s or pad with zeros."""
    a = np.asarray(audio, np.float32).reshape(-1)
    return a[:length] if a.size >= length else np.concatenate([a, np.zeros(length - a.size, np.float32)])


def collect_heads(model, tokenizer, clips: Iterable[Tuple[np.ndarray, str]], *, session=None, z_threshold: float = 3.0,
                  counts: Optional[dict] = None):
    """-> (votes [L, H], strengths [L, H]): the means over the surveyed clips of fold_clip's results.  ``clips`` yields
    (16 kHz float32 waveform, transcript).  A clip whose token row exceeds n_text_ctx is skipped, logged and counted
    (``counts``, when given, receives {"used", "skipped"}); ValueError when none is left.  ``session``: a beam-1 session
    of ``model`` outside the batch engine (``new_session(batched=False)``); one is made and closed here otherwise."""
    dims = model.dims
    own = session is None
    sess = model.new_session(beam=1, batched=False) if own else session
    votes = np.zeros((dims.n_text_layer, dims.n_text_head), np.float64)
    strengths = np.zeros_like(votes)
    used = skipped = 0
    try:
        for audio, transcript in clips:
            tokens = survey_tokens(tokenizer, transcript)
            if len(tokens) > dims.n_text_ctx:
                skipped += 1
                logger.warning("alignment heads: clip skipped, %d tokens exceed the text context of %d", len(tokens), dims.n_text_ctx)
                continue
            mel = sess.log_mel(pad_or_trim_audio(audio))
            sess.encode_mel(mel[:, :N_FRAMES])
            peaks, _ = sess.head_survey(tokens, mel.shape[-1])
            strength, vote = fold_clip(peaks, z_threshold)
            strengths += strength
            votes += vote
            used += 1
    finally:
        if own:
            sess.close()
    if counts is not None:
        counts.update(used=used, skipped=skipped)
    if used == 0:
        raise ValueError("alignment heads: no clip left to survey")
    return votes / used, strengths / used


def select_heads(strengths, votes=None, *, min_strength: float = 0.05, min_votes: Optional[float] = None) -> np.ndarray:
    """bool [L, H]: the reference's rule ``strengths > 0.05`` (:286); with ``min_votes`` the alternative it carries
    commented out, ``votes > min_votes`` (:285)."""
    if min_votes is not None:
        if votes is None:
            raise ValueError("select_heads: min_votes needs the votes")
        return np.asarray(votes) > min_votes
    return np.asarray(strengths) > min_strength


# ---- command line ------------------------------------------------------------------------------------------------
def read_audio(path: str) -> np.ndarray:
    if path.lower().endswith(".npy"):
        a = np.load(path)
        if a.dtype != np.float32:
            raise ValueError(f"{path}: expected float32 samples, got {a.dtype}")
        return a.reshape(-1)
    with wave.open(path, "rb") as w:
        if w.getframerate() != SAMPLE_RATE or w.getnchannels() != 1 or w.getsampwidth() != 2:
            raise ValueError(f"{path}: expected 16 kHz mono 16-bit PCM")
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
    return pcm.astype(np.float32) / 32768.0


def read_manifest(path: str) -> List[Tuple[np.ndarray, str]]:
    base = os.path.dirname(os.path.abspath(path))
    clips = []
    with open(path, encoding="utf-8") as fh:
        for n, line in enumerate(fh, 1):
            if not line.strip():
                continue
            entry = json.loads(line)
            if "audio" not in entry or "text" not in entry:
                raise ValueError(f"{path}:{n}: expected {{\"audio\": ..., \"text\": ...}}")
            clips.append((read_audio(os.path.join(base, entry["audio"])), str(entry["text"])))
    return clips


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m whisperlivekit_amd.alignment_heads", description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", required=True, help="local checkpoint: file or directory")
    ap.add_argument("--lora", default=None, help="LoRA adapter merged at load")
    ap.add_argument("--clips", required=True, help="manifest, one JSON object per line")
    ap.add_argument("--language", default="en")
    ap.add_argument("--min-strength", type=float, default=0.05)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--output", default="alignment_heads.b85")
    args = ap.parse_args(argv)

    from .checkpoint import load_whisper_checkpoint
    from .engine import HipWhisperModel
    from .tokenizer import get_tokenizer
    dims, sd, _ = load_whisper_checkpoint(args.model, args.lora)
    model = HipWhisperModel.from_state_dict(dims, sd, [], args.device)      # the survey reads no head table
    try:
        tokenizer = get_tokenizer(dims.is_multilingual, num_languages=dims.num_languages, language=args.language,
                                  task="transcribe")
        counts = {}
        votes, strengths = collect_heads(model, tokenizer, read_manifest(args.clips), counts=counts)
    finally:
        model.close()
    mask = select_heads(strengths, votes, min_strength=args.min_strength)
    with open(args.output, "w", encoding="ascii") as fh:
        fh.write(dump_mask(mask))
    print(f"{int(mask.sum())} of {mask.size} heads selected (strength > {args.min_strength}), {counts['skipped']} clips skipped -> {args.output}")
    print("pairs:", " ".join(f"{l},{h}" for l, h in mask_pairs(mask)))
    print("strength (votes) per layer:")
    for l in range(dims.n_text_layer):
        print(f"  layer {l:2d}: " + " ".join(f"{strengths[l, h]:.3f}{'*' if mask[l, h] else ' '}({votes[l, h]:.2f})"
                                             for h in range(dims.n_text_head)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
