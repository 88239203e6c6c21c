"""Thin Python objects over the C ABI: one :class:`HipWhisperModel` per GPU (immutable packed
weights, shared by every session on that GPU) and one :class:`HipSession` per audio stream
(device-resident rolling audio, KV caches, alignment window, HIP stream)."""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Dict, Iterable, List, Mapping, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .dims import ALIGNMENT_HEADS, MODEL_DIMS, ModelDims, default_alignment_heads
from .melbank import mel_filterbank


def _as_f32(x) -> np.ndarray:
    if hasattr(x, "detach"):  # torch tensor
        x = x.detach().cpu().float().numpy()
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32))


def hann_window_periodic(n: int = 400) -> np.ndarray:
    """torch.hann_window(n) (periodic).  Uses torch when importable so the fp32 values are the
    very ones whisper/audio.py:147 multiplies with."""
    try:
        import torch
        return torch.hann_window(n).numpy().astype(np.float32)
    except Exception:  # pragma: no cover
        k = np.arange(n, dtype=np.float64)
        return (0.5 - 0.5 * np.cos(2.0 * np.pi * k / n)).astype(np.float32)


def pack_state_dict(dims: ModelDims, sd: Mapping[str, object]) -> Dict[str, np.ndarray]:
    """Reference checkpoint names (whisper/model.py module tree, as produced by load_model,
    whisper/__init__.py:466-596) -> the packed tensors wlk_tensor_lookup() defines.

    * conv weights [out, in, tap] become tap-major [out, tap*in] rows (the conv is a GEMM over a
      time-major activation buffer);
    * query/key/value (key has no bias, model.py:89) are concatenated into one [3d, d] projection,
      cross-attention key/value into one [2d, d] projection."""
    g = lambda k: _as_f32(sd[k])
    out: Dict[str, np.ndarray] = {}
    out["mel.filters"] = np.ascontiguousarray(mel_filterbank(dims.n_mels))
    out["mel.window"] = hann_window_periodic()
    d = dims.n_audio_state
    out["enc.conv1.w"] = np.ascontiguousarray(g("encoder.conv1.weight").transpose(0, 2, 1).reshape(d, -1))
    out["enc.conv1.b"] = g("encoder.conv1.bias")
    out["enc.conv2.w"] = np.ascontiguousarray(g("encoder.conv2.weight").transpose(0, 2, 1).reshape(d, -1))
    out["enc.conv2.b"] = g("encoder.conv2.bias")
    out["enc.pos"] = g("encoder.positional_embedding")

    def block(dst: str, src: str, width: int, cross: bool):
        zeros = np.zeros(width, np.float32)
        a = src + ".attn"
        out[dst + "ln1.w"], out[dst + "ln1.b"] = g(src + ".attn_ln.weight"), g(src + ".attn_ln.bias")
        out[dst + "qkv.w"] = np.concatenate([g(a + ".query.weight"), g(a + ".key.weight"), g(a + ".value.weight")])
        out[dst + "qkv.b"] = np.concatenate([g(a + ".query.bias"), zeros, g(a + ".value.bias")])
        out[dst + "out.w"], out[dst + "out.b"] = g(a + ".out.weight"), g(a + ".out.bias")
        if cross:
            x = src + ".cross_attn"
            out[dst + "lnx.w"], out[dst + "lnx.b"] = g(src + ".cross_attn_ln.weight"), g(src + ".cross_attn_ln.bias")
            out[dst + "xq.w"], out[dst + "xq.b"] = g(x + ".query.weight"), g(x + ".query.bias")
            out[dst + "xkv.w"] = np.concatenate([g(x + ".key.weight"), g(x + ".value.weight")])
            out[dst + "xkv.b"] = np.concatenate([zeros, g(x + ".value.bias")])
            out[dst + "xout.w"], out[dst + "xout.b"] = g(x + ".out.weight"), g(x + ".out.bias")
        out[dst + "ln2.w"], out[dst + "ln2.b"] = g(src + ".mlp_ln.weight"), g(src + ".mlp_ln.bias")
        out[dst + "fc1.w"], out[dst + "fc1.b"] = g(src + ".mlp.0.weight"), g(src + ".mlp.0.bias")
        out[dst + "fc2.w"], out[dst + "fc2.b"] = g(src + ".mlp.2.weight"), g(src + ".mlp.2.bias")

    for i in range(dims.n_audio_layer):
        block(f"enc.{i}.", f"encoder.blocks.{i}", dims.n_audio_state, cross=False)
    out["enc.ln_post.w"], out["enc.ln_post.b"] = g("encoder.ln_post.weight"), g("encoder.ln_post.bias")
    out["dec.tok_emb"] = g("decoder.token_embedding.weight")
    out["dec.pos"] = g("decoder.positional_embedding")
    for i in range(dims.n_text_layer):
        block(f"dec.{i}.", f"decoder.blocks.{i}", dims.n_text_state, cross=True)
    out["dec.ln.w"], out["dec.ln.b"] = g("decoder.ln.weight"), g("decoder.ln.bias")
    return {k: np.ascontiguousarray(v.reshape(-1)) for k, v in out.items()}


def _cdims(dims: ModelDims) -> _lib.Dims:
    return _lib.Dims(*dims.as_tuple())


def arena_floats(dims: ModelDims) -> int:
    n = C.c_uint64()
    _lib.check(_lib.load().wlk_arena_floats(C.byref(_cdims(dims)), C.byref(n)))
    return int(n.value)


def packed_tensor_names(dims: ModelDims) -> List[str]:
    lib = _lib.load()
    names, i = [], 0
    cd = _cdims(dims)
    while True:
        s = C.c_char_p()
        if lib.wlk_tensor_name(C.byref(cd), i, C.byref(s)) != 0:
            break
        names.append(s.value.decode())
        i += 1
    return names


class HipWhisperModel:
    """Packed fp32 weights of one Whisper checkpoint resident on one GPU."""
    _wlk_hip_model = True

    def __init__(self, dims: ModelDims, device: int = 0, arena=None):
        """``arena``: optional torch CUDA float32 tensor of ``arena_floats(dims)`` elements that the
        caller owns (torch.distributed broadcasts it over RCCL); otherwise the library allocates."""
        self.lib = _lib.load()
        self.dims = dims
        self.device = device
        self._arena_keepalive = arena
        self._h = C.c_void_p()
        ptr = None
        if arena is not None:
            if arena.numel() != arena_floats(dims) or str(arena.dtype) != "torch.float32" or not arena.is_cuda:
                raise ValueError("arena must be a CUDA float32 tensor of arena_floats(dims) elements")
            ptr = C.c_void_p(arena.data_ptr())
        _lib.check(self.lib.wlk_model_create(C.byref(_cdims(dims)), device, ptr, C.byref(self._h)))
        self.alignment_heads: List[Tuple[int, int]] = []
        self.finalized = False
        # CIF end-of-word head on the device (opt-in; align_att.cif_device_enabled): the switch, and which checkpoint the
        # first session put there
        self.cif_device = False
        self._cif_lock = threading.Lock()
        self._cif_path: Optional[str] = None
        # the reference's AlignAttBase._base_init reads len(model.decoder.blocks) (align_att_base.py:58)
        import types
        self.decoder = types.SimpleNamespace(blocks=[None] * dims.n_text_layer)

    # -- weights --------------------------------------------------------------------------
    def upload_packed(self, packed: Mapping[str, np.ndarray]) -> None:
        expected = set(packed_tensor_names(self.dims))
        missing = expected - set(packed)
        if missing:
            raise KeyError(f"missing packed tensors: {sorted(missing)[:5]} ...")
        for name in expected:
            a = np.ascontiguousarray(packed[name], dtype=np.float32).reshape(-1)
            _lib.check(self.lib.wlk_model_upload(self._h, name.encode(), a.ctypes.data_as(C.c_void_p), a.size))

    def load_state_dict(self, sd: Mapping[str, object]) -> None:
        self.upload_packed(pack_state_dict(self.dims, sd))

    def set_alignment_heads(self, pairs: Sequence[Tuple[int, int]]) -> None:
        flat = np.asarray([x for p in pairs for x in p], dtype=np.int32)
        _lib.check(self.lib.wlk_model_set_alignment_heads(self._h, flat.ctypes.data_as(C.c_void_p), len(pairs)))
        self.alignment_heads = [tuple(p) for p in pairs]

    def finalize(self) -> None:
        _lib.check(self.lib.wlk_model_finalize(self._h))
        self.finalized = True

    @classmethod
    def from_state_dict(cls, dims: ModelDims, sd: Mapping[str, object],
                        alignment_heads: Optional[Sequence[Tuple[int, int]]] = None, device: int = 0,
                        arena=None) -> "HipWhisperModel":
        m = cls(dims, device, arena)
        m.load_state_dict(sd)
        m.set_alignment_heads(alignment_heads if alignment_heads is not None else default_alignment_heads(dims))
        m.finalize()
        return m

    @classmethod
    def synthetic(cls, name: str, seed: int = 0, device: int = 0) -> "HipWhisperModel":
        """Seeded random weights of a named architecture (no checkpoint / network needed)."""
        from . import synth
        dims = MODEL_DIMS[name]
        return cls.from_state_dict(dims, synth.synth_state_dict(dims, seed), ALIGNMENT_HEADS[name], device)

    # -- reference-compatible read-only attributes (whisper/model.py:385-395) ----------------
    @property
    def is_multilingual(self) -> bool:
        return self.dims.is_multilingual

    @property
    def num_languages(self) -> int:
        return self.dims.num_languages

    def new_session(self, beam: int = 1, max_audio_seconds: float = 64.0, batched: Optional[bool] = None) -> "HipSession":
        """``batched`` (default: on for beam 1 unless WLK_BATCH_DECODE=0): the session's decode loops share batched
        single-token steps with the other sessions of this GPU (wlk_engine_attach)."""
        s = HipSession(self, beam, int(max_audio_seconds * 16000))
        if batched is None:
            batched = beam == 1 and os.environ.get("WLK_BATCH_DECODE", "1") != "0"
        if batched:
            s.attach_engine()
        return s

    def set_cif(self, weight, bias: float = 0.0) -> None:
        """Put the CIF end-of-word head (a Linear(n_audio_state, 1): ``weight`` [d], ``bias``) on the device beside the
        weights: every later encode of this model's sessions leaves the head's decision on the device
        (:meth:`HipSession.cif_result`).  ``weight=None`` removes it.  Not while an encode of this model is running."""
        if weight is None:
            _lib.check(self.lib.wlk_model_set_cif(self._h, None, 0, 0.0))
            return
        w = _as_f32(weight).reshape(-1)
        _lib.check(self.lib.wlk_model_set_cif(self._h, w.ctypes.data_as(C.c_void_p), w.size, float(bias)))

    def ensure_cif(self, path: str, weight, bias: float) -> None:
        """Called by every session that uses the device CIF head: the first one uploads it (under the model's lock,
        before that session's first encode); a later session configured with another checkpoint is refused - the head
        belongs to the shared model."""
        key = os.path.abspath(str(path))
        with self._cif_lock:
            if self._cif_path is None:
                self.set_cif(weight, bias)
                self._cif_path = key
            elif self._cif_path != key:
                raise ValueError(f"this model's device CIF head was loaded from {self._cif_path}; a session asked for "
                                 f"{key} (one head per shared model)")

    def engine_stats(self) -> Dict[str, int]:
        """Iterations of this GPU's batch engine and the rows (= session steps) advanced in them."""
        v = [C.c_uint64() for _ in range(4)]
        _lib.check(self.lib.wlk_engine_stats(self._h, *[C.byref(x) for x in v]))
        it, rows, bs, br = (int(x.value) for x in v)
        eb, es = C.c_uint64(), C.c_uint64()
        _lib.check(self.lib.wlk_engine_encode_stats(self._h, C.byref(eb), C.byref(es)))
        pb, ps = C.c_uint64(), C.c_uint64()
        _lib.check(self.lib.wlk_engine_prefill_stats(self._h, C.byref(pb), C.byref(ps)))
        return dict(iterations=it, rows=rows, batched_steps=bs, batched_rows=br,
                    mean_rows_per_batched_step=round(br / bs, 3) if bs else None,
                    encode_batches=int(eb.value), encoded_sessions=int(es.value),
                    mean_sessions_per_encode_batch=round(es.value / eb.value, 3) if eb.value else None,
                    prefill_batches=int(pb.value), stacked_prefills=int(ps.value),
                    mean_sessions_per_prefill_batch=round(ps.value / pb.value, 3) if pb.value else None)

    def close(self) -> None:
        # sessions the batch path (transcribe.py) keeps per calling thread hold pointers into this model
        for rows in (self.__dict__.pop("_batch_rows", None) or {}).values():
            for sess in rows.sessions.values():
                sess.close()
        stacker = self.__dict__.pop("_window_stacker", None)      # transcribe.WindowStacker: its group holds this model
        if stacker is not None:
            stacker.close()
        if self._h:
            self.lib.wlk_model_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class LoopOutcome:
    """What wlk_decode_until_stop / wlk_job_result hand back, as plain Python values."""
    __slots__ = ("new_tokens", "step_tokens", "step_frames", "step_sum_logprobs", "stop_reason", "last_attend_frame",
                 "no_speech_prob", "sum_logprob", "decode_calls")

    def __init__(self, res: "_lib.LoopResult", new, step_tokens, step_frames, step_sums):
        n, k = int(res.n_steps), int(res.n_new_tokens)
        self.new_tokens = [int(x) for x in new[:k]]
        self.step_tokens = [int(x) for x in step_tokens[:n]]
        self.step_frames = [int(x) for x in step_frames[:n]]
        self.step_sum_logprobs = [float(x) for x in step_sums[:n]]
        self.stop_reason = int(res.stop_reason)
        self.last_attend_frame = int(res.last_attend_frame)
        self.no_speech_prob = float(res.no_speech_prob)
        self.sum_logprob = float(res.sum_logprob)
        self.decode_calls = int(res.decode_calls)


class HipSession:
    """Per-stream device state.  One call in flight at a time (the reference's threading
    contract for a session); different sessions may be driven from different threads."""

    def __init__(self, model: HipWhisperModel, beam: int = 1, max_audio_samples: int = 64 * 16000):
        if not model.finalized:
            raise _lib.WlkError("model must be finalized before creating sessions")
        self.model = model
        self.lib = model.lib
        self.beam = beam
        self._h = C.c_void_p()
        _lib.check(self.lib.wlk_session_create(model._h, beam, max_audio_samples, C.byref(self._h)))
        self.max_audio_samples = max_audio_samples
        self.export_calls: Dict[str, int] = {}      # wlk_export calls by name (tests pin what stays on the device)

    # -- audio (a1) -------------------------------------------------------------------------
    def append(self, pcm: np.ndarray) -> None:
        a = np.ascontiguousarray(pcm, dtype=np.float32).reshape(-1)
        _lib.check(self.lib.wlk_audio_append(self._h, a.ctypes.data_as(C.c_void_p), a.size))

    def append_pcm16(self, pcm: np.ndarray) -> None:
        """int16 samples as they arrive on the wire; widened to fp32 / 32768 on the device."""
        a = np.ascontiguousarray(pcm, dtype=np.int16).reshape(-1)
        _lib.check(self.lib.wlk_audio_append_pcm16(self._h, a.ctypes.data_as(C.c_void_p), a.size))

    def append_zeros(self, n: int) -> None:
        _lib.check(self.lib.wlk_audio_append_zeros(self._h, int(n)))

    def drop_front(self, n: int) -> None:
        _lib.check(self.lib.wlk_audio_drop_front(self._h, int(n)))

    def clear_audio(self) -> None:
        _lib.check(self.lib.wlk_audio_clear(self._h))

    @property
    def audio_len(self) -> int:
        n = C.c_int()
        _lib.check(self.lib.wlk_audio_len(self._h, C.byref(n)))
        return n.value

    # -- hot path ---------------------------------------------------------------------------
    def encode(self) -> int:
        cml = C.c_int32()
        _lib.check(self.lib.wlk_encode(self._h, C.byref(cml)))
        return cml.value

    def cif_result(self) -> "_lib.CifOut":
        """The device CIF head's record of the last encode (wlk_cif_result): ``fire`` is the end-of-word decision.
        Waits for the encode only if its record has not arrived yet."""
        out = _lib.CifOut()
        _lib.check(self.lib.wlk_cif_result(self._h, C.byref(out)))
        return out

    def encode_mel(self, mel: np.ndarray) -> None:
        """Encode a [n_mels, 3000] log-mel segment as whisper.transcribe() / find_alignment hand it to the model
        (instead of the session's own audio): encoder + cross-K/V."""
        mel = np.ascontiguousarray(_as_f32(mel))
        if mel.shape != (self.model.dims.n_mels, 3000):
            raise ValueError(f"encode_mel: expected [{self.model.dims.n_mels}, 3000], got {mel.shape}")
        _lib.check(self.lib.wlk_encode_mel(self._h, mel.ctypes.data_as(C.POINTER(C.c_float)), 3000))

    def log_mel(self, audio: np.ndarray, padding: int = 0) -> np.ndarray:
        """whisper/audio.py:log_mel_spectrogram(audio, n_mels, padding) of a whole recording -> [n_mels, frames]."""
        a = np.ascontiguousarray(_as_f32(audio)).reshape(-1)
        n = C.c_int32()
        _lib.check(self.lib.wlk_log_mel(self._h, None, a.size, int(padding), None, 0, C.byref(n)))
        out = np.empty((self.model.dims.n_mels, n.value), np.float32)
        _lib.check(self.lib.wlk_log_mel(self._h, a.ctypes.data_as(C.POINTER(C.c_float)), a.size, int(padding),
                                        out.ctypes.data_as(C.POINTER(C.c_float)), out.size, C.byref(n)))
        return out

    def find_alignment(self, tokens: Sequence[int], n_sot: int, eot: int, num_frames: int, qk_scale: float = 1.0,
                       want_cost: bool = False):
        """Device half of whisper/timing.py:find_alignment on the encoded session.  ``tokens`` = [sot sequence (n_sot
        ids), <|notimestamps|>, text tokens, <|endoftext|>].  -> (dtw step codes [(n_text + 2), num_frames // 2 + 1],
        token probabilities [n_text], cost matrix [n_text + 1, num_frames // 2] or None)."""
        toks = np.ascontiguousarray(np.asarray(tokens, dtype=np.int64))
        n_text = len(toks) - n_sot - 2
        if n_text < 1:
            raise ValueError("find_alignment: no text tokens")
        f = num_frames // 2
        trace = np.empty((n_text + 2, f + 1), dtype=np.int8)
        probs = np.empty(n_text, dtype=np.float32)
        cost = np.empty((n_text + 1, f), dtype=np.float32) if want_cost else None
        _lib.check(self.lib.wlk_find_alignment(
            self._h, toks.ctypes.data_as(C.POINTER(C.c_int64)), len(toks), int(n_sot), int(eot), int(num_frames),
            float(qk_scale), cost.ctypes.data_as(C.POINTER(C.c_float)) if want_cost else None,
            trace.ctypes.data_as(C.POINTER(C.c_int8)), probs.ctypes.data_as(C.POINTER(C.c_float))))
        return trace, probs, cost

    def head_survey(self, tokens: Sequence[int], num_frames: int = 3000) -> Tuple[np.ndarray, np.ndarray]:
        """One teacher-forced decoder pass over ``tokens`` on the encoded session; for EVERY decoder layer and head the peak
        of softmax(cross-attention scores[:num_frames // 2]) of every token row and the position that attains it
        (wlk_head_survey; scripts/determine_alignment_heads.py:149-168 of the reference).
        -> (peaks [n_text_layer, n_text_head, P] float32, frames [same] int32).  The session needs a new prefill afterwards."""
        toks = np.ascontiguousarray(np.asarray(tokens, dtype=np.int64).reshape(-1))
        d = self.model.dims
        shape = (d.n_text_layer, d.n_text_head, max(len(toks), 1))
        peaks, frames = np.empty(shape, np.float32), np.empty(shape, np.int32)
        _lib.check(self.lib.wlk_head_survey(self._h, toks.ctypes.data_as(C.POINTER(C.c_int64)), len(toks), int(num_frames),
                                            peaks.ctypes.data_as(C.POINTER(C.c_float)), frames.ctypes.data_as(C.POINTER(C.c_int32))))
        return peaks, frames

    def decode(self, tokens: np.ndarray, first: bool, sot_index: int = 0) -> None:
        t = np.ascontiguousarray(tokens, dtype=np.int64)
        if t.ndim != 2:
            raise ValueError("tokens must be [rows, n_tok]")
        _lib.check(self.lib.wlk_decode(self._h, t.ctypes.data_as(C.c_void_p), t.shape[0], t.shape[1],
                                       1 if first else 0, int(sot_index)))

    def no_speech_prob(self, token: int) -> np.ndarray:
        out = np.empty(self.beam, np.float32)
        _lib.check(self.lib.wlk_no_speech_prob(self._h, int(token), out.ctypes.data_as(C.c_void_p)))
        return out

    def set_rules(self, suppressed: Sequence[int], blank: Sequence[int]) -> None:
        """The token lists of whisper's SuppressTokens / SuppressBlank for wlk_pick_greedy (decoding.py:417-432)."""
        a = np.ascontiguousarray(suppressed, dtype=np.int32).reshape(-1)
        b = np.ascontiguousarray(blank, dtype=np.int32).reshape(-1)
        key = (a.tobytes(), b.tobytes())
        if key == getattr(self, "_rules_key", None):
            return              # this mask is the one on the device: no drain of the stream, no upload (one per 30 s window)
        _lib.check(self.lib.wlk_rules_set(self._h, a.ctypes.data_as(C.c_void_p), a.size, b.ctypes.data_as(C.c_void_p), b.size))
        self._rules_key = key

    def pick_greedy(self, *, first_step: bool, without_timestamps: bool, timestamp_begin: int, eot: int, no_timestamps: int,
                    ts_mode: int, ts_bound: int, max_initial: int) -> Tuple[int, float]:
        """Logit rules + argmax + log-probability of the last decode's row on the device (decoding.py:270-287, 417-499)."""
        prm = np.asarray([int(first_step), int(without_timestamps), timestamp_begin, eot, no_timestamps, ts_mode, ts_bound,
                          max_initial], dtype=np.int32)
        tok = np.empty(1, np.int32)
        lp = np.empty(1, np.float32)
        _lib.check(self.lib.wlk_pick_greedy(self._h, prm.ctypes.data_as(C.c_void_p), tok.ctypes.data_as(C.c_void_p),
                                            lp.ctypes.data_as(C.c_void_p)))
        return int(tok[0]), float(lp[0])

    PICK_FIELDS = ("first_step", "without_timestamps", "timestamp_begin", "eot", "no_timestamps", "ts_mode", "ts_bound",
                   "max_initial")

    def pick_topk(self, states: Sequence[dict], k: int) -> Tuple[np.ndarray, np.ndarray]:
        """Logit rules + log-softmax + the k best of every row of the last decode on the device (wlk_pick_topk): ``states``
        holds one dictionary of pick_greedy's keywords per row.  -> (log-probabilities [rows, k], ids [rows, k])."""
        prm = np.asarray([[int(st[f]) for f in self.PICK_FIELDS] for st in states], dtype=np.int32).reshape(-1, 8)
        n, kk = prm.shape[0], max(int(k), 0)
        lp = np.empty((n, kk), np.float32)
        ids = np.empty((n, kk), np.int32)
        _lib.check(self.lib.wlk_pick_topk(self._h, prm.ctypes.data_as(C.c_void_p), n, int(k), lp.ctypes.data_as(C.c_void_p),
                                          ids.ctypes.data_as(C.c_void_p)))
        return lp, ids

    def decode_ancestry(self, last_tokens: Sequence[int], sources: Sequence[int]) -> None:
        """One single-token step whose row b continues hypothesis sources[b] of the previous step (wlk_decode_ancestry):
        kv_reorder(sources) + decode(last_tokens) without moving the cache where the session qualifies."""
        t = np.ascontiguousarray(last_tokens, dtype=np.int64).reshape(-1)
        src = np.ascontiguousarray(sources, dtype=np.int32).reshape(-1)
        if src.size != t.size:
            raise ValueError("decode_ancestry: one source row per token")
        _lib.check(self.lib.wlk_decode_ancestry(self._h, t.ctypes.data_as(C.c_void_p), src.ctypes.data_as(C.c_void_p), t.size))

    def select(self, adj_rows: Sequence[int], adj_ids: Sequence[int], adj_deltas: Sequence[float], k: int,
               content_mel_len: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        n = len(adj_ids)
        r = np.asarray(adj_rows, dtype=np.int32)
        i = np.asarray(adj_ids, dtype=np.int32)
        dl = np.asarray(adj_deltas, dtype=np.float32)
        lp = np.empty((self.beam, k), np.float32)
        ids = np.empty((self.beam, k), np.int32)
        fr = np.empty(self.beam, np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        _lib.check(self.lib.wlk_select(self._h, vp(r), vp(i), vp(dl), n, k, int(content_mel_len), vp(lp), vp(ids),
                                       vp(fr)))
        return lp, ids, fr

    def decode_until_stop(self, tokens: Sequence[int], params: "_lib.LoopParams", suppress_ids: Sequence[int],
                          blank_ids: Sequence[int]) -> "LoopOutcome":
        """The whole AlignAtt decode loop of one infer (beam 1) in one library call (wlk_decode_until_stop)."""
        t = np.ascontiguousarray(tokens, dtype=np.int64).reshape(-1)
        sup = np.ascontiguousarray(suppress_ids, dtype=np.int32)
        blank = np.ascontiguousarray(blank_ids, dtype=np.int32)
        cap = int(params.max_text_len) + 8
        res = _lib.LoopResult()
        new = np.empty(cap, np.int64)
        st, sf = np.empty(cap, np.int32), np.empty(cap, np.int32)
        ss = np.empty(cap, np.float32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        _lib.check(self.lib.wlk_decode_until_stop(self._h, vp(t), t.size, C.byref(params), vp(sup), sup.size, vp(blank),
                                                  blank.size, C.byref(res), vp(new), vp(st), vp(sf), vp(ss), cap))
        return LoopOutcome(res, new, st, sf, ss)

    def decode_beam_until_stop(self, tokens: Sequence[int], params: "_lib.LoopParams", suppress_ids: Sequence[int],
                               blank_ids: Sequence[int]) -> "LoopOutcome":
        """The same loop for the beam decoder, beams 2-7 (wlk_decode_beam_until_stop); ``tokens`` is one row's prompt."""
        t = np.ascontiguousarray(tokens, dtype=np.int64).reshape(-1)
        sup = np.ascontiguousarray(suppress_ids, dtype=np.int32)
        blank = np.ascontiguousarray(blank_ids, dtype=np.int32)
        cap = int(params.max_text_len) + 8
        res = _lib.LoopResult()
        new = np.empty(cap, np.int64)
        st, sf = np.empty(cap, np.int32), np.empty(cap, np.int32)
        ss = np.empty(cap, np.float32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        _lib.check(self.lib.wlk_decode_beam_until_stop(self._h, vp(t), t.size, C.byref(params), vp(sup), sup.size, vp(blank),
                                                       blank.size, C.byref(res), vp(new), vp(st), vp(sf), vp(ss), cap))
        return LoopOutcome(res, new, st, sf, ss)

    def beam_step(self, tokens: Sequence[int], source_rows: Sequence[int]) -> None:
        """Diagnostic: one single-token forward over the beam ancestry table (wlk_diag_beam_step)."""
        t = np.ascontiguousarray(tokens, dtype=np.int64).reshape(-1)
        src = np.ascontiguousarray(source_rows, dtype=np.int32).reshape(-1)
        _lib.check(self.lib.wlk_diag_beam_step(self._h, t.ctypes.data_as(C.c_void_p), src.ctypes.data_as(C.c_void_p), t.size))

    def beam_stats(self) -> Dict[str, int]:
        """Single-token steps of this session that ran over the ancestry table (wlk_session_beam_stats)."""
        n = C.c_uint64()
        _lib.check(self.lib.wlk_session_beam_stats(self._h, C.byref(n)))
        return dict(ancestry_steps=int(n.value))

    def attach_engine(self) -> None:
        _lib.check(self.lib.wlk_engine_attach(self._h))

    def detach_engine(self) -> None:
        _lib.check(self.lib.wlk_engine_detach(self._h))

    def kv_reorder(self, source_rows: Sequence[int]) -> None:
        s = np.asarray(source_rows, dtype=np.int32)
        _lib.check(self.lib.wlk_kv_reorder(self._h, s.ctypes.data_as(C.c_void_p), s.size))

    def sync(self) -> None:
        _lib.check(self.lib.wlk_sync(self._h))

    # -- parity / profiling -------------------------------------------------------------------
    def set_debug(self, on: bool = True) -> None:
        _lib.check(self.lib.wlk_session_set_debug(self._h, 1 if on else 0))

    def export(self, what: str, max_floats: Optional[int] = None) -> np.ndarray:
        d = self.model.dims
        if max_floats is None:
            max_floats = max(d.n_mels * 3000, 1500 * d.n_audio_state, self.beam * d.n_vocab,
                             self.beam * d.n_text_ctx * d.n_text_head * 1500)
        buf = np.empty(max_floats, np.float32)
        n = C.c_uint64()
        self.export_calls[what] = self.export_calls.get(what, 0) + 1
        _lib.check(self.lib.wlk_export(self._h, what.encode(), buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(n)))
        return buf[: n.value].copy()

    def step_stats(self) -> Dict[str, float]:
        """Wall time of this session's graph-replayed single-token steps so far (wlk_session_step_stats)."""
        n, wall, launch = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _lib.check(self.lib.wlk_session_step_stats(self._h, C.byref(n), C.byref(wall), C.byref(launch)))
        return dict(steps=int(n.value), wall_ns=int(wall.value), launch_ns=int(launch.value))

    def prof_begin(self) -> None:
        _lib.check(self.lib.wlk_prof_begin(self._h))

    def prof_end(self, cap: int = 64) -> Dict[str, Dict[str, float]]:
        """-> {launch tag: {"ms", "launches", "flops", "bytes"}} summed since prof_begin()."""
        names = (C.c_char_p * cap)()
        ms = np.zeros(cap, np.float32)
        cnt = np.zeros(cap, np.int32)
        fl = np.zeros(cap, np.float64)
        by = np.zeros(cap, np.float64)
        n = C.c_int32()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        _lib.check(self.lib.wlk_prof_end(self._h, cap, names, vp(ms), vp(cnt), vp(fl), vp(by), C.byref(n)))
        return {names[i].decode(): dict(ms=float(ms[i]), launches=int(cnt[i]), flops=float(fl[i]), bytes=float(by[i]))
                for i in range(n.value)}

    def close(self) -> None:
        if self._h:
            self.lib.wlk_session_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class HipWindowGroup:
    """A wlk_group (csrc/window_group.hip): the greedy temperature-0 steps of up to ``rows`` batch-Whisper windows, each in
    its own prefilled beam-1 :class:`HipSession` of ``model``, as one launch chain per token.  One step at a time."""

    def __init__(self, model: HipWhisperModel, rows: int = 8):
        self.model = model
        self.lib = model.lib
        self.rows = int(rows)
        self._h = C.c_void_p()
        _lib.check(self.lib.wlk_group_create(model._h, self.rows, C.byref(self._h)))

    def step_pick(self, sessions: Sequence[HipSession], tokens: Sequence[int], states: Sequence[dict]
                  ) -> Tuple[np.ndarray, np.ndarray]:
        """Feeds ``tokens[r]`` to ``sessions[r]`` and picks each row's next token under that session's rules and
        ``states[r]`` (the keywords of :meth:`HipSession.pick_greedy`).  -> (token ids [n] int32, log-probabilities [n])."""
        n = len(sessions)
        handles = (C.c_void_p * max(n, 1))(*[s._h for s in sessions])
        tok = np.ascontiguousarray(tokens, dtype=np.int64).reshape(-1)
        prm = np.asarray([[int(st[f]) for f in HipSession.PICK_FIELDS] for st in states], dtype=np.int32).reshape(-1, 8)
        if tok.size != n or prm.shape[0] != n:
            raise ValueError("step_pick: one token and one rule state per session")
        out = np.empty(max(n, 1), np.int32)
        lp = np.empty(max(n, 1), np.float32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        _lib.check(self.lib.wlk_group_step_pick(self._h, handles, vp(tok), vp(prm), n, vp(out), vp(lp)))
        return out[:n], lp[:n]

    def run_pick(self, sessions: Sequence[HipSession], tokens: Sequence[int], states: Sequence[dict],
                 max_steps: Sequence[int], burst: int) -> List[Tuple[np.ndarray, np.ndarray]]:
        """wlk_group_run_pick: up to ``burst`` (1..16) steps of every row behind one call.  Row r feeds ``tokens[r]``, then
        its own picks, for at most ``max_steps[r]`` steps (and no further than <|endoftext|> or the text context); the rule
        states advance on the device from ``states[r]``.  -> per row (token ids int32 [steps_r], log-probabilities float32
        [steps_r]): what ``steps_r`` successive :meth:`step_pick` calls return."""
        n, burst = len(sessions), int(burst)
        handles = (C.c_void_p * max(n, 1))(*[s._h for s in sessions])
        tok = np.ascontiguousarray(tokens, dtype=np.int64).reshape(-1)
        prm = np.asarray([[int(st[f]) for f in HipSession.PICK_FIELDS] for st in states], dtype=np.int32).reshape(-1, 8)
        lim = np.ascontiguousarray(max_steps, dtype=np.int32).reshape(-1)
        if tok.size != n or prm.shape[0] != n or lim.size != n:
            raise ValueError("run_pick: one token, one rule state and one step budget per session")
        width = max(burst, 1)
        out = np.zeros((max(n, 1), width), np.int32)
        lp = np.zeros((max(n, 1), width), np.float32)
        steps = np.zeros(max(n, 1), np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        _lib.check(self.lib.wlk_group_run_pick(self._h, handles, vp(tok), vp(prm), vp(lim), n, burst, vp(out), vp(lp), vp(steps)))
        return [(out[r, :steps[r]].copy(), lp[r, :steps[r]].copy()) for r in range(n)]

    def find_alignment(self, windows: Sequence[tuple], want_cost: bool = False, want_trace: bool = False) -> List[tuple]:
        """wlk_group_find_alignment: the device half of whisper/timing.py:find_alignment for up to ``rows`` windows in one
        stacked pass.  ``windows``: (session, tokens, n_sot, eot, num_frames[, qk_scale]) each, ``tokens`` = [sot sequence,
        <|notimestamps|>, text tokens, <|endoftext|>] and the session encoded.  -> per window (starts [n_text + 1] int32 -
        the frame at which the path enters each text row, the last one <|endoftext|>'s -, token probabilities [n_text],
        cost matrix or None, dtw step codes or None).  Afterwards every session needs a new prefill."""
        n = len(windows)
        arr = (_lib.AlignWindow * max(n, 1))()
        keep, out = [], []
        vp = lambda a: a.ctypes.data_as(C.c_void_p).value
        for a, win in zip(arr, windows):
            sess, tokens, n_sot, eot, num_frames = win[:5]
            toks = np.ascontiguousarray(np.asarray(tokens, dtype=np.int64).reshape(-1))
            n_text, f = max(len(toks) - int(n_sot) - 2, 0), max(int(num_frames) // 2, 0)
            starts = np.empty(n_text + 1, np.int32)
            probs = np.empty(max(n_text, 1), np.float32)
            cost = np.empty((n_text + 1, f), np.float32) if want_cost else None
            trace = np.empty((n_text + 2, f + 1), np.int8) if want_trace else None
            a.s, a.tokens, a.n_tokens, a.n_sot, a.eot, a.num_frames = sess._h, vp(toks), len(toks), int(n_sot), int(eot), int(num_frames)
            a.qk_scale = float(win[5]) if len(win) > 5 else 1.0
            a.starts, a.token_probs = vp(starts), vp(probs)
            a.cost, a.trace = (vp(cost) if want_cost else None), (vp(trace) if want_trace else None)
            keep.append(toks)
            out.append((starts, probs[:n_text], cost, trace))
        _lib.check(self.lib.wlk_group_find_alignment(self._h, arr, n))
        return out

    def fits(self, n_tokens: int, num_frames: int) -> bool:
        """wlk_group_align_fits: can a window of ``n_tokens`` tokens (sot sequence, <|notimestamps|>, text, <|endoftext|>) over
        ``num_frames`` mel frames ride in :meth:`find_alignment`?  A pure host function of the shape and the model."""
        ok = C.c_int32()
        _lib.check(self.lib.wlk_group_align_fits(self._h, int(n_tokens), int(num_frames), C.byref(ok)))
        return bool(ok.value)

    def verify(self, windows: Sequence[tuple], want_picks: bool = False) -> List[dict]:
        """wlk_group_verify: how far greedy decoding at temperature 0 follows each window's draft, in ONE teacher-forced
        decoder pass over all windows.  ``windows``: (session, initial tokens, draft tokens, sot_index, first-pick state,
        no_speech_token or None) each, the session encoded and with ``set_rules`` lists.  -> per window a dict: ``accepted``
        (k), ``next_token`` and ``next_logprob`` (the pick behind draft[:k]), ``sum_logprob`` (positions 0..k, added in that
        order in float32), ``no_speech_prob``, and with ``want_picks`` (tests) ``picks`` = (token ids int32 [n_d + 1],
        log-probabilities float32 [n_d + 1]) of every candidate position.  Afterwards each session is what its own prefill
        of initial + draft[:k] leaves."""
        n = len(windows)
        arr = (_lib.VerifyWindow * max(n, 1))()
        res = (_lib.VerifyResult * max(n, 1))()
        keep, picks = [], []
        vp = lambda a: a.ctypes.data_as(C.c_void_p).value
        for i, (a, win) in enumerate(zip(arr, windows)):
            sess, initial, draft, sot_index, state, no_speech = win
            initial = [int(t) for t in initial]
            draft = [int(t) for t in draft]
            toks = np.ascontiguousarray(np.asarray(initial + draft, dtype=np.int64).reshape(-1))
            a.s, a.tokens, a.n_initial, a.n_tokens = sess._h, vp(toks), len(initial), len(toks)
            a.sot_index, a.no_speech_token = int(sot_index), -1 if no_speech is None else int(no_speech)
            a.p = (C.c_int32 * 8)(*[int(state[f]) for f in HipSession.PICK_FIELDS])
            a.result = C.pointer(res[i])
            pk = np.zeros((len(draft) + 1, 2), np.int32) if want_picks else None
            a.picks = vp(pk) if want_picks else None
            keep.append(toks)
            picks.append(pk)
        _lib.check(self.lib.wlk_group_verify(self._h, arr, n))
        out = []
        for r, pk in zip(res[:n], picks):
            o = dict(accepted=int(r.accepted), next_token=int(r.next_token), next_logprob=np.float32(r.next_logprob),
                     sum_logprob=np.float32(r.sum_logprob), no_speech_prob=float(r.no_speech_prob))
            if pk is not None:
                o["picks"] = (pk[:, 0].copy(), pk[:, 1].copy().view(np.float32))
            out.append(o)
        return out

    def verify_fits(self, n_initial: int, n_draft: int) -> bool:
        """wlk_group_verify_fits: can a window of ``n_initial`` initial and ``n_draft`` draft tokens ride in :meth:`verify`?
        A pure host function of the shape and the model."""
        ok = C.c_int32()
        _lib.check(self.lib.wlk_group_verify_fits(self._h, int(n_initial), int(n_draft), C.byref(ok)))
        return bool(ok.value)

    def stats(self) -> Dict[str, float]:
        steps, rows = C.c_uint64(), C.c_uint64()
        _lib.check(self.lib.wlk_group_stats(self._h, C.byref(steps), C.byref(rows)))
        return dict(steps=int(steps.value), rows=int(rows.value),
                    mean_rows_per_step=round(rows.value / steps.value, 3) if steps.value else None)

    def export_logits(self, row: int) -> np.ndarray:
        """The logits row of slot ``row`` of the last step (tests)."""
        buf = np.empty(self.model.dims.n_vocab, np.float32)
        n = C.c_uint64()
        _lib.check(self.lib.wlk_group_export_logits(self._h, int(row), buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(n)))
        return buf[: n.value]

    def close(self) -> None:
        if self._h:
            self.lib.wlk_group_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def pick_rows(logits: np.ndarray, masks: np.ndarray, mask_of_row: Sequence[int], states: Sequence[dict]
              ) -> Tuple[np.ndarray, np.ndarray]:
    """wlk_diag_pick_rows (tests): the rows pick kernel on host logits [n, V] and rule masks [n_masks, V] uint8."""
    lib = _lib.load()
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    mk = np.ascontiguousarray(masks, dtype=np.uint8)
    mo = np.ascontiguousarray(mask_of_row, dtype=np.int32)
    prm = np.asarray([[int(st[f]) for f in HipSession.PICK_FIELDS] for st in states], dtype=np.int32).reshape(-1, 8)
    n = lg.shape[0]
    out = np.empty(n, np.int32)
    lp = np.empty(n, np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    _lib.check(lib.wlk_diag_pick_rows(vp(lg), lg.shape[1], vp(mk), mk.shape[0], vp(mo), vp(prm), n, vp(out), vp(lp)))
    return out, lp


def pick_one(logits: np.ndarray, mask: np.ndarray, state: dict) -> Tuple[int, np.float32]:
    """wlk_diag_pick_one (tests): the one-row pick kernel of ``HipSession.pick_greedy`` on a host logits row [V], one rule
    mask [V] uint8 and one rule state.  -> (token, log-probability with the kernel's bits)."""
    lib = _lib.load()
    lg = np.ascontiguousarray(logits, dtype=np.float32).reshape(-1)
    mk = np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1)
    if mk.size != lg.size:
        raise ValueError("pick_one: a logits row [V] and a mask [V]")
    prm = np.asarray([int(state[f]) for f in HipSession.PICK_FIELDS], dtype=np.int32)
    tok = np.empty(1, np.int32)
    lp = np.empty(1, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    _lib.check(lib.wlk_diag_pick_one(vp(lg), lg.size, vp(mk), vp(prm), vp(tok), vp(lp)))
    return int(tok[0]), lp.view(np.float32)[0]


def pick_topk_rows(logits: np.ndarray, mask: np.ndarray, states: Sequence[dict], k: int) -> Tuple[np.ndarray, np.ndarray]:
    """wlk_diag_pick_topk (tests): the top-k kernel of ``HipSession.pick_topk`` on host logits [n, V], one rule mask [V]
    uint8 and one rule state per row.  -> (log-probabilities [n, k], ids [n, k])."""
    lib = _lib.load()
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    mk = np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1)
    prm = np.asarray([[int(st[f]) for f in HipSession.PICK_FIELDS] for st in states], dtype=np.int32).reshape(-1, 8)
    if lg.ndim != 2 or lg.shape[0] != prm.shape[0] or mk.size != lg.shape[1]:
        raise ValueError("pick_topk_rows: logits [n, V], a mask [V] and n states")
    n, kk = lg.shape[0], max(int(k), 0)
    lp = np.empty((n, kk), np.float32)
    ids = np.empty((n, kk), np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    _lib.check(lib.wlk_diag_pick_topk(vp(lg), lg.shape[1], vp(mk), vp(prm), n, int(k), vp(lp), vp(ids)))
    return lp, ids


def draft_pick(logits: np.ndarray, mask: np.ndarray, state: dict, draft: Sequence[int], ended: bool = False
               ) -> Tuple[np.ndarray, np.ndarray, dict]:
    """wlk_diag_draft_pick (tests): the two kernels behind ``HipWindowGroup.verify``'s decoder pass on host logits
    [len(draft) + 1, V], one rule mask [V] uint8 and the first position's rule state.  -> (token ids, log-probabilities
    of every position, dict(accepted, next_token, next_logprob, sum_logprob))."""
    lib = _lib.load()
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    mk = np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1)
    dr = np.ascontiguousarray(draft, dtype=np.int32).reshape(-1)
    if lg.ndim != 2 or lg.shape[0] != dr.size + 1 or mk.size != lg.shape[1]:
        raise ValueError("draft_pick: logits [len(draft) + 1, V] and a mask [V]")
    prm = np.asarray([int(state[f]) for f in HipSession.PICK_FIELDS], dtype=np.int32)
    out = np.empty(lg.shape[0], np.int32)
    lp = np.empty(lg.shape[0], np.float32)
    res = _lib.VerifyResult()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    _lib.check(lib.wlk_diag_draft_pick(vp(lg), lg.shape[1], vp(mk), vp(prm), vp(dr), dr.size, int(bool(ended)), vp(out), vp(lp),
                                       C.byref(res)))
    return out, lp, dict(accepted=int(res.accepted), next_token=int(res.next_token), next_logprob=np.float32(res.next_logprob),
                         sum_logprob=np.float32(res.sum_logprob))


def pick_advance(states: Sequence[dict], tokens: Sequence[int]) -> List[dict]:
    """wlk_diag_pick_advance (tests): the device form of the rule transition, one (state, picked token) pair per entry.
    -> the next states, integers throughout (``first_step`` and ``without_timestamps`` as 0 / 1)."""
    lib = _lib.load()
    prm = np.asarray([[int(st[f]) for f in HipSession.PICK_FIELDS] for st in states], dtype=np.int32).reshape(-1, 8)
    tok = np.ascontiguousarray(tokens, dtype=np.int32).reshape(-1)
    if tok.size != prm.shape[0]:
        raise ValueError("pick_advance: one token per state")
    out = np.zeros_like(prm)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    _lib.check(lib.wlk_diag_pick_advance(vp(prm), vp(tok), tok.size, vp(out)))
    return [dict(zip(HipSession.PICK_FIELDS, (int(v) for v in row))) for row in out]
