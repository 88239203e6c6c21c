"""NLLB-200 (M2M-100 architecture) on the HIP library: the translation model of config 5.

The reference reaches this model through the third-party ``nllw`` package (``whisperlivekit/core.py:320-329``
``nllw.load_model``; ``core.py:483-493`` / ``translation.py`` wrap it in ``nllw.OnlineTranslation``).  ``nllw`` is not in the
reference tree; what it executes is the published M2M-100 network of ``transformers``
(``models/m2m_100/modeling_m2m_100.py``) or its CTranslate2 conversion, selected per call by ``forced_bos_token_id`` = the
target language code.  This module is that network behind the C ABI (``wlk_nllb_*``, csrc/nllb.hip) with

* :func:`pack_hf_state_dict` - a ``transformers`` checkpoint's tensors (``model.shared.weight``,
  ``model.encoder.layers.N.self_attn.q_proj.weight`` ...) into the packed arena;
* :class:`HipNllbModel` / :class:`HipNllbSession` - encoder pass, decoder steps with KV cache, beam reorder, top-k;
* :class:`HipNllbBatch` / :func:`generate_batch` - up to 8 DIFFERENT sentences per launch chain (csrc/nllb_batch.hip):
  ``generate`` on a padded batch in ``transformers``, without the padding - greedy decoding of any number of sentences
  through the slots of one batch, every token position one stacked step;
* :func:`generate_alignatt` - AlignAtt streaming decoding (opt-in): the decoder's cross-attention
  says which source token a target token leans on, and a token that leans on the unstable end of the source is held back;
* :func:`generate` / :func:`beam_search` - ``GenerationMixin.generate`` for the cases the translation backends use: greedy
  or beam search from ``[decoder_start_token_id]`` with the target language forced as the first generated token and
  ``</s>`` ending a hypothesis.

Pinned by ``transformers``' own ``M2M100ForConditionalGeneration`` on seeded weights (``scripts/gen_golden_nllb.py``,
``tests/golden/nllb_kat.npz``).  The streaming policy of ``nllw.OnlineTranslation`` (when to re-translate which prefix) is
host logic of that package and is not restated.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import Callable, Dict, Iterable, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib


@dataclass(frozen=True)
class NllbConfig:
    """The fields of ``M2M100Config`` the network depends on."""
    vocab_size: int = 256206
    d_model: int = 1024
    encoder_layers: int = 12
    decoder_layers: int = 12
    attention_heads: int = 16
    ffn_dim: int = 4096
    scale_embedding: bool = True
    pad_token_id: int = 1
    eos_token_id: int = 2
    decoder_start_token_id: int = 2
    max_position_embeddings: int = 1024


NLLB_200_DISTILLED_600M = NllbConfig()
NLLB_MICRO = NllbConfig(vocab_size=2003, d_model=128, encoder_layers=2, decoder_layers=2, attention_heads=2, ffn_dim=256,
                        max_position_embeddings=96)


def sinusoid_table(n_rows: int, d: int, padding_idx: Optional[int]) -> np.ndarray:
    """``M2M100SinusoidalPositionalEmbedding.get_embedding`` (tensor2tensor flavour: all sines, then all cosines; the
    padding row zeroed), computed with torch's float32 operators so that the table is the one ``transformers`` builds."""
    import torch
    half = d // 2
    step = math.log(10000) / (half - 1)
    freq = torch.exp(torch.arange(half, dtype=torch.int64).float() * -step)
    ang = torch.arange(n_rows, dtype=torch.int64).float().unsqueeze(1) * freq.unsqueeze(0)
    table = torch.cat([torch.sin(ang), torch.cos(ang)], dim=1).view(n_rows, -1)
    if d % 2 == 1:
        table = torch.cat([table, torch.zeros(n_rows, 1)], dim=1)
    if padding_idx is not None:
        table[padding_idx, :] = 0
    return table.numpy().astype(np.float32)


def _f32(x) -> np.ndarray:
    if hasattr(x, "detach"):
        x = x.detach().cpu().float().numpy()
    return np.ascontiguousarray(x, dtype=np.float32)


def pack_hf_state_dict(cfg: NllbConfig, sd: Mapping[str, object], n_positions: int) -> Dict[str, np.ndarray]:
    """``transformers`` parameter names -> packed names (include/wlk_hip.h).  q / k / v projections are stacked row-wise."""
    out: Dict[str, np.ndarray] = {}
    shared = sd.get("model.shared.weight")
    if shared is None:
        shared = sd.get("lm_head.weight", sd.get("model.encoder.embed_tokens.weight"))
    if shared is None:
        raise KeyError("no shared embedding in the state dict (model.shared.weight / lm_head.weight)")
    out["shared.emb"] = _f32(shared)
    out["pos.table"] = sinusoid_table(n_positions, cfg.d_model, cfg.pad_token_id)

    def lin(prefix):
        return _f32(sd[prefix + ".weight"]), _f32(sd[prefix + ".bias"])

    def block(dst: str, src: str, cross: bool):
        for ours, theirs in (("ln1", "self_attn_layer_norm"), ("ln2", "final_layer_norm"), ("fc1", "fc1"), ("fc2", "fc2"),
                             ("out", "self_attn.out_proj")):
            out[dst + ours + ".w"], out[dst + ours + ".b"] = lin(src + theirs)
        q, k, v = (lin(src + "self_attn." + n + "_proj") for n in "qkv")
        out[dst + "qkv.w"] = np.concatenate([q[0], k[0], v[0]], axis=0)
        out[dst + "qkv.b"] = np.concatenate([q[1], k[1], v[1]], axis=0)
        if cross:
            out[dst + "lnx.w"], out[dst + "lnx.b"] = lin(src + "encoder_attn_layer_norm")
            out[dst + "xq.w"], out[dst + "xq.b"] = lin(src + "encoder_attn.q_proj")
            k, v = (lin(src + "encoder_attn." + n + "_proj") for n in "kv")
            out[dst + "xkv.w"] = np.concatenate([k[0], v[0]], axis=0)
            out[dst + "xkv.b"] = np.concatenate([k[1], v[1]], axis=0)
            out[dst + "xout.w"], out[dst + "xout.b"] = lin(src + "encoder_attn.out_proj")

    for i in range(cfg.encoder_layers):
        block(f"enc.{i}.", f"model.encoder.layers.{i}.", False)
    for i in range(cfg.decoder_layers):
        block(f"dec.{i}.", f"model.decoder.layers.{i}.", True)
    out["enc.ln.w"], out["enc.ln.b"] = lin("model.encoder.layer_norm")
    out["dec.ln.w"], out["dec.ln.b"] = lin("model.decoder.layer_norm")
    return out


def synth_state_dict(cfg: NllbConfig, seed: int = 0, eos_gain: float = 2.0) -> Dict[str, np.ndarray]:
    """Seeded random parameters under the ``transformers`` names (there is no checkpoint and no network where this is
    built and measured).  Linear weights ~ N(0, 1/fan_in), biases ~ N(0, 0.02^2), LayerNorm gains ~ 1 + N(0, 0.1^2),
    embedding ~ N(0, 0.04 / d_model) (small next to the layers' contributions: with a tied output projection a large
    embedding makes every random-weight generation repeat its last token); the ``</s>`` row is scaled by ``eos_gain`` so
    that generations end now and then."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd: Dict[str, np.ndarray] = {}
    d, f = cfg.d_model, cfg.ffn_dim

    def normal(shape, std):
        return (rng.standard_normal(shape, dtype=np.float32) * np.float32(std)).astype(np.float32)

    def linear(name, n_out, n_in):
        sd[name + ".weight"] = normal((n_out, n_in), 1.0 / np.sqrt(n_in))
        sd[name + ".bias"] = normal((n_out,), 0.02)

    def layernorm(name):
        sd[name + ".weight"] = (1.0 + normal((d,), 0.1)).astype(np.float32)
        sd[name + ".bias"] = normal((d,), 0.02)

    emb = normal((cfg.vocab_size, d), 0.2 / np.sqrt(d))
    emb[cfg.eos_token_id] *= np.float32(eos_gain)
    sd["model.shared.weight"] = emb
    for side, n, cross in (("encoder", cfg.encoder_layers, False), ("decoder", cfg.decoder_layers, True)):
        for i in range(n):
            p = f"model.{side}.layers.{i}."
            for proj in ("q_proj", "k_proj", "v_proj", "out_proj"):
                linear(p + "self_attn." + proj, d, d)
            layernorm(p + "self_attn_layer_norm")
            if cross:
                for proj in ("q_proj", "k_proj", "v_proj", "out_proj"):
                    linear(p + "encoder_attn." + proj, d, d)
                layernorm(p + "encoder_attn_layer_norm")
            linear(p + "fc1", f, d)
            linear(p + "fc2", d, f)
            layernorm(p + "final_layer_norm")
        layernorm(f"model.{side}.layer_norm")
    return sd


class HipNllbModel:
    """Packed weights of one NLLB / M2M-100 network on one GPU."""

    def __init__(self, cfg: NllbConfig, device: int = 0, max_src: int = 256, max_tgt: int = 256):
        self.lib = _lib.load()
        self.cfg = cfg
        self.device = device
        n_pos = max(max_src, max_tgt) + cfg.pad_token_id + 2
        self.cdims = _lib.NllbDims(cfg.vocab_size, cfg.d_model, cfg.attention_heads, cfg.ffn_dim, cfg.encoder_layers,
                                   cfg.decoder_layers, max_src, max_tgt, cfg.pad_token_id, n_pos,
                                   math.sqrt(cfg.d_model) if cfg.scale_embedding else 1.0)
        self.n_positions = n_pos
        self._h = C.c_void_p()
        _lib.check(self.lib.wlk_nllb_create(C.byref(self.cdims), device, C.byref(self._h)))
        self.finalized = False

    def upload_packed(self, packed: Mapping[str, np.ndarray]) -> None:
        for name, arr in packed.items():
            a = np.ascontiguousarray(arr, dtype=np.float32)
            _lib.check(self.lib.wlk_nllb_upload(self._h, name.encode(), a.ctypes.data_as(C.c_void_p), a.size))
        _lib.check(self.lib.wlk_nllb_finalize(self._h))
        self.finalized = True

    @classmethod
    def from_hf_state_dict(cls, cfg: NllbConfig, sd: Mapping[str, object], device: int = 0, max_src: int = 256,
                           max_tgt: int = 256) -> "HipNllbModel":
        m = cls(cfg, device, max_src, max_tgt)
        m.upload_packed(pack_hf_state_dict(cfg, sd, m.n_positions))
        return m

    @classmethod
    def synthetic(cls, cfg: NllbConfig, seed: int = 0, device: int = 0, **kw) -> "HipNllbModel":
        return cls.from_hf_state_dict(cfg, synth_state_dict(cfg, seed), device, **kw)

    def new_session(self, rows: int = 1) -> "HipNllbSession":
        return HipNllbSession(self, rows)

    def new_batch(self, n_slots: int = 8) -> "HipNllbBatch":
        return HipNllbBatch(self, n_slots)

    def close(self) -> None:
        if self._h:
            self.lib.wlk_nllb_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class HipNllbSession:
    """Device state of one translation request: encoder output, cross K/V, the self-attention caches of ``rows`` hypotheses."""

    def __init__(self, model: HipNllbModel, rows: int = 1):
        if not model.finalized:
            raise _lib.WlkError("NLLB model must be finalized before creating sessions")
        self.model, self.lib, self.rows = model, model.lib, rows
        self._h = C.c_void_p()
        _lib.check(self.lib.wlk_nllb_session_create(model._h, rows, C.byref(self._h)))

    def encode(self, src_ids: Sequence[int]) -> None:
        a = np.ascontiguousarray(src_ids, dtype=np.int64).reshape(-1)
        _lib.check(self.lib.wlk_nllb_encode(self._h, a.ctypes.data_as(C.c_void_p), a.size))

    def decode(self, tokens, first: bool) -> None:
        t = np.ascontiguousarray(tokens, dtype=np.int64)
        if t.ndim != 2:
            raise ValueError("tokens must be [rows, n_tok]")
        _lib.check(self.lib.wlk_nllb_decode(self._h, t.ctypes.data_as(C.c_void_p), t.shape[0], t.shape[1], 1 if first else 0))

    def step(self, tokens: Sequence[int], k: int = 1) -> Tuple[np.ndarray, np.ndarray]:
        """One token per row after the prompt + the k best continuations of every row, one graph replay (wlk_nllb_step)."""
        t = np.ascontiguousarray(tokens, dtype=np.int64).reshape(-1)
        lp = np.empty((self.rows, k), np.float32)
        ids = np.empty((self.rows, k), np.int32)
        _lib.check(self.lib.wlk_nllb_step(self._h, t.ctypes.data_as(C.c_void_p), t.size, k, lp.ctypes.data_as(C.c_void_p),
                                          ids.ctypes.data_as(C.c_void_p)))
        return lp, ids

    def kv_reorder(self, source_rows: Sequence[int]) -> None:
        a = np.ascontiguousarray(source_rows, dtype=np.int32)
        _lib.check(self.lib.wlk_nllb_kv_reorder(self._h, a.ctypes.data_as(C.c_void_p), a.size))

    def step_beam(self, tokens: Sequence[int], sources: Sequence[int], k: int) -> Tuple[np.ndarray, np.ndarray]:
        """Beam step without moving the cache (wlk_nllb_step_beam): row i continues the hypothesis row ``sources[i]`` held
        after the previous step and is fed ``tokens[i]``; the k (1..16) best continuations of every row, one graph replay.
        After it ``step`` / ``decode(first=False)`` / ``kv_reorder`` are errors until the next ``decode(first=True)``."""
        t = np.ascontiguousarray(tokens, dtype=np.int64).reshape(-1)
        src = np.ascontiguousarray(sources, dtype=np.int32).reshape(-1)
        if src.size != t.size:
            raise ValueError("step_beam: one source row per token")
        lp = np.empty((self.rows, k), np.float32)
        ids = np.empty((self.rows, k), np.int32)
        _lib.check(self.lib.wlk_nllb_step_beam(self._h, t.ctypes.data_as(C.c_void_p), src.ctypes.data_as(C.c_void_p), t.size, k,
                                               lp.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p)))
        return lp, ids

    def beam_stats(self) -> Dict[str, int]:
        n = C.c_uint64()
        _lib.check(self.lib.wlk_nllb_session_beam_stats(self._h, C.byref(n)))
        return {"ancestry_steps": int(n.value)}

    def set_alignment_heads(self, pairs: Sequence[Tuple[int, int]]) -> None:
        """The ``(decoder layer, head)`` pairs (1..64, no duplicates) whose cross-attention ``step_align`` reads; an empty
        list switches the read-out off.  The order is the order the heads are summed in."""
        a = np.ascontiguousarray([tuple(int(v) for v in pr) for pr in pairs], dtype=np.int32).reshape(-1, 2)
        _lib.check(self.lib.wlk_nllb_session_set_align(self._h, a.ctypes.data_as(C.c_void_p), a.shape[0]))

    def step_align(self, tokens: Sequence[int], k: int, lo: int, hi: int, limit: int):
        """``step`` + the alignment read-out, one graph replay (wlk_nllb_step_align) -> ``(logprobs [rows, k], ids [rows, k],
        pos [rows], prob [rows], mass [rows])``: with ``p`` the mean of the selected heads' softmax rows over the source,
        ``pos`` = the first arg-max of ``p[lo:hi]`` (-1: empty window), ``prob`` = ``p[pos]``, ``mass`` = ``p[limit:].sum()``."""
        t = np.ascontiguousarray(tokens, dtype=np.int64).reshape(-1)
        lp = np.empty((self.rows, k), np.float32)
        ids = np.empty((self.rows, k), np.int32)
        pos = np.empty(self.rows, np.int32)
        prob = np.empty(self.rows, np.float32)
        mass = np.empty(self.rows, np.float32)
        _lib.check(self.lib.wlk_nllb_step_align(self._h, t.ctypes.data_as(C.c_void_p), t.size, k, int(lo), int(hi), int(limit),
                                                *(a.ctypes.data_as(C.c_void_p) for a in (lp, ids, pos, prob, mass))))
        return lp, ids, pos, prob, mass

    def alignment(self) -> np.ndarray:
        """``p [rows, src_len]`` of the latest ``step_align``."""
        return self._export("align", self.rows * self.model.cdims.max_src).reshape(self.rows, -1)

    def align_stats(self) -> Dict[str, int]:
        steps, captures = C.c_uint64(), C.c_uint64()
        _lib.check(self.lib.wlk_nllb_session_align_stats(self._h, C.byref(steps), C.byref(captures)))
        return {"align_steps": int(steps.value), "graph_captures": int(captures.value)}

    def generate_alignatt_loop(self, prompt: Sequence[int], n_accessible: int, threshold: int, final: bool, eos_id: int,
                               max_new: int) -> Tuple[List[int], List[int], str]:
        """wlk_nllb_generate_alignatt: the loop of :func:`generate_alignatt` inside the library, after ``encode``."""
        pr = np.ascontiguousarray(prompt, dtype=np.int64).reshape(-1)
        out = np.empty(max(int(max_new), 1), np.int64)
        al = np.empty(max(int(max_new), 1), np.int32)
        n, why = C.c_int32(), C.c_int32()
        _lib.check(self.lib.wlk_nllb_generate_alignatt(self._h, pr.ctypes.data_as(C.c_void_p), pr.size, int(n_accessible),
                                                       int(threshold), 1 if final else 0, int(eos_id), int(max_new),
                                                       out.ctypes.data_as(C.c_void_p), al.ctypes.data_as(C.c_void_p),
                                                       C.byref(n), C.byref(why)))
        return out[: n.value].tolist(), al[: n.value].tolist(), _lib.ALIGN_STOP_REASONS[why.value]

    def topk(self, k: int) -> Tuple[np.ndarray, np.ndarray]:
        """The k (1..16) best log-probabilities and ids of every row of the latest decode; k > 8 takes the wide kernel."""
        lp = np.empty((self.rows, k), np.float32)
        ids = np.empty((self.rows, k), np.int32)
        _lib.check(self.lib.wlk_nllb_topk(self._h, k, lp.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p)))
        return lp, ids

    def _export(self, what: str, n: int) -> np.ndarray:
        buf = np.empty(n, np.float32)
        got = C.c_uint64()
        _lib.check(self.lib.wlk_nllb_export(self._h, what.encode(), buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(got)))
        return buf[: got.value]

    def logits(self) -> np.ndarray:
        return self._export("logits", self.rows * self.model.cfg.vocab_size).reshape(self.rows, -1)

    def encoder_output(self) -> np.ndarray:
        return self._export("enc", self.model.cdims.max_src * self.model.cfg.d_model).reshape(-1, self.model.cfg.d_model)

    def sync(self) -> None:
        _lib.check(self.lib.wlk_nllb_sync(self._h))

    def close(self) -> None:
        if self._h:
            self.lib.wlk_nllb_session_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class HipNllbBatch:
    """Device state of up to ``n_slots`` (1..8) sentences in flight, stepped together (``wlk_nllb_batch_*``): every slot has
    its own encoder output, cross K/V, self-attention cache and lengths; one step feeds one token to any subset of the
    slots and streams the decoder's weights once for all of them.  One caller at a time."""

    def __init__(self, model: HipNllbModel, n_slots: int = 8):
        if not model.finalized:
            raise _lib.WlkError("NLLB model must be finalized before creating batches")
        self.model, self.lib, self.n_slots = model, model.lib, int(n_slots)
        self._h = C.c_void_p()
        _lib.check(self.lib.wlk_nllb_batch_create(model._h, self.n_slots, C.byref(self._h)))

    def encode(self, slots: Sequence[int], sources: Sequence[Sequence[int]]) -> None:
        """One stacked ragged encoder pass: ``sources[i]`` (unpadded ids) into slot ``slots[i]``; other slots are untouched."""
        if len(slots) != len(sources):
            raise ValueError("encode: one source per slot")
        sl = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        arrs = [np.asarray(s, dtype=np.int64).reshape(-1) for s in sources]
        off = np.zeros(len(arrs) + 1, np.int32)
        off[1:] = np.cumsum([a.size for a in arrs])
        ids = np.ascontiguousarray(np.concatenate(arrs) if arrs else np.zeros(0, np.int64))
        _lib.check(self.lib.wlk_nllb_batch_encode(self._h, sl.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p),
                                                  off.ctypes.data_as(C.c_void_p), sl.size))

    def step(self, slots: Sequence[int], tokens: Sequence[int], k: int = 1) -> Tuple[np.ndarray, np.ndarray]:
        """One token per named slot (at most one row per slot, any subset, any order) -> the k best log-probabilities and
        ids of every row, ``[len(slots), k]``.  A slot's first step after its encode feeds the decoder start token."""
        sl = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        t = np.ascontiguousarray(tokens, dtype=np.int64).reshape(-1)
        if sl.size != t.size:
            raise ValueError("step: one token per slot")
        lp = np.empty((sl.size, k), np.float32)
        ids = np.empty((sl.size, k), np.int32)
        _lib.check(self.lib.wlk_nllb_batch_step(self._h, sl.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), sl.size, k,
                                                lp.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p)))
        return lp, ids

    def set_alignment_heads(self, pairs: Sequence[Tuple[int, int]]) -> None:
        """The ``(decoder layer, head)`` pairs (1..64, no duplicates) ``step_align`` reads, for every slot; an empty list
        switches the read-out off.  Nothing is allocated or recorded before the first ``step_align``."""
        a = np.ascontiguousarray([tuple(int(v) for v in pr) for pr in pairs], dtype=np.int32).reshape(-1, 2)
        _lib.check(self.lib.wlk_nllb_batch_set_align(self._h, a.ctypes.data_as(C.c_void_p), a.shape[0]))

    def prefill(self, slots: Sequence[int], prompts: Sequence[Sequence[int]]) -> None:
        """One stacked decoder pass over the prompts of freshly encoded slots (wlk_nllb_batch_prefill): ``prompts[i]`` (at
        least one id, at most ``max_tgt - 1``) fills positions ``0 .. len - 1`` of slot ``slots[i]``; no logits are formed -
        the next token of a slot goes through ``step`` / ``step_align``."""
        if len(slots) != len(prompts):
            raise ValueError("prefill: one prompt per slot")
        sl = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        arrs = [np.asarray(pr, dtype=np.int64).reshape(-1) for pr in prompts]
        off = np.zeros(len(arrs) + 1, np.int32)
        off[1:] = np.cumsum([a.size for a in arrs])
        ids = np.ascontiguousarray(np.concatenate(arrs) if arrs else np.zeros(0, np.int64))
        _lib.check(self.lib.wlk_nllb_batch_prefill(self._h, sl.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p),
                                                   off.ctypes.data_as(C.c_void_p), sl.size))

    def verify(self, slots: Sequence[int], token_lists: Sequence[Sequence[int]]) -> Tuple[np.ndarray, np.ndarray]:
        """Draft verification of freshly encoded slots in ONE stacked decoder pass (wlk_nllb_batch_verify, DESIGN.md section
        31): ``token_lists[i] = [decoder start, forced first token, d_0 .. d_{n-1}]`` -> ``(accepted int32 [len(slots)],
        next_token int64 [len(slots)])``: the greedy picks agree with the first ``accepted[i]`` draft tokens, and
        ``next_token[i]`` is the pick behind them.  The slot then holds ``2 + accepted[i]`` target tokens and continues with
        ``step`` feeding ``next_token[i]``."""
        if len(slots) != len(token_lists):
            raise ValueError("verify: one token list per slot")
        sl = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        arrs = [np.asarray(t, dtype=np.int64).reshape(-1) for t in token_lists]
        off = np.zeros(len(arrs) + 1, np.int32)
        off[1:] = np.cumsum([a.size for a in arrs])
        ids = np.ascontiguousarray(np.concatenate(arrs) if arrs else np.zeros(0, np.int64))
        accepted, nxt = np.empty(sl.size, np.int32), np.empty(sl.size, np.int64)
        _lib.check(self.lib.wlk_nllb_batch_verify(self._h, sl.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p),
                                                  off.ctypes.data_as(C.c_void_p), sl.size, accepted.ctypes.data_as(C.c_void_p),
                                                  nxt.ctypes.data_as(C.c_void_p)))
        return accepted, nxt

    def verify_stats(self) -> Dict[str, int]:
        passes, draft, accepted = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _lib.check(self.lib.wlk_nllb_batch_verify_stats(self._h, C.byref(passes), C.byref(draft), C.byref(accepted)))
        return {"passes": int(passes.value), "draft_tokens": int(draft.value), "accepted_tokens": int(accepted.value)}

    def step_align(self, slots: Sequence[int], tokens: Sequence[int], k: int, lo: Sequence[int], hi: Sequence[int],
                   limit: Sequence[int]):
        """``step`` + the alignment read-out of every row, one graph replay (wlk_nllb_batch_step_align) -> ``(logprobs
        [rows, k], ids [rows, k], pos [rows], prob [rows], mass [rows])``; row r has its own window ``lo[r], hi[r]`` and
        ``limit[r]`` over its own source (``HipNllbSession.step_align`` per row).  Every slot named holds a prompt already."""
        sl = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        t = np.ascontiguousarray(tokens, dtype=np.int64).reshape(-1)
        win = [np.ascontiguousarray(w, dtype=np.int32).reshape(-1) for w in (lo, hi, limit)]
        if any(a.size != sl.size for a in [t] + win):
            raise ValueError("step_align: one token and one lo / hi / limit per slot")
        n = sl.size
        lp, ids = np.empty((n, k), np.float32), np.empty((n, k), np.int32)
        pos, prob, mass = np.empty(n, np.int32), np.empty(n, np.float32), np.empty(n, np.float32)
        _lib.check(self.lib.wlk_nllb_batch_step_align(self._h, sl.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), n, int(k),
                                                      *(a.ctypes.data_as(C.c_void_p) for a in win + [lp, ids, pos, prob, mass])))
        return lp, ids, pos, prob, mass

    def alignment(self, slot: int) -> np.ndarray:
        """``p [src_len]`` of the slot's row in the latest ``step_align``."""
        return self._export(slot, "align", self.model.cdims.max_src)

    def align_stats(self) -> Dict[str, int]:
        steps, captures = C.c_uint64(), C.c_uint64()
        _lib.check(self.lib.wlk_nllb_batch_align_stats(self._h, C.byref(steps), C.byref(captures)))
        return {"align_steps": int(steps.value), "graph_captures": int(captures.value)}

    def release(self, slot: int) -> None:
        _lib.check(self.lib.wlk_nllb_batch_release(self._h, int(slot)))

    def _export(self, slot: int, what: str, n: int) -> np.ndarray:
        buf = np.empty(n, np.float32)
        got = C.c_uint64()
        _lib.check(self.lib.wlk_nllb_batch_export(self._h, int(slot), what.encode(), buf.ctypes.data_as(C.c_void_p), buf.size,
                                                  C.byref(got)))
        return buf[: got.value]

    def encoder_output(self, slot: int) -> np.ndarray:
        return self._export(slot, "enc", self.model.cdims.max_src * self.model.cfg.d_model).reshape(-1, self.model.cfg.d_model)

    def logits(self, slot: int) -> np.ndarray:
        """The slot's row of the latest step's logits, ``[vocab]``."""
        return self._export(slot, "logits", self.model.cfg.vocab_size)

    def cross_attention(self, slots: Sequence[int], layer: int, q: np.ndarray) -> np.ndarray:
        """Diagnostics: the ragged cross-attention kernel alone, queries ``q [len(slots), d_model]`` (pre-scaled) against the
        named slots' cross K/V of decoder layer ``layer``."""
        sl = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        qa = np.ascontiguousarray(q, dtype=np.float32)
        if qa.shape != (sl.size, self.model.cfg.d_model):
            raise ValueError("cross_attention: q must be [len(slots), d_model]")
        out = np.empty_like(qa)
        _lib.check(self.lib.wlk_nllb_batch_cross_attention(self._h, sl.ctypes.data_as(C.c_void_p), sl.size, int(layer),
                                                           qa.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
        return out

    def sync(self) -> None:
        _lib.check(self.lib.wlk_nllb_batch_sync(self._h))

    def close(self) -> None:
        if self._h:
            self.lib.wlk_nllb_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def generate(session, src_ids: Sequence[int], forced_bos_token_id: Optional[int] = None, *, max_new_tokens: int = 199,
             forced_eos_token_id: Optional[int] = None) -> List[int]:
    """``model.generate(input_ids, forced_bos_token_id=<target language>, num_beams=1, do_sample=False,
    max_new_tokens=n)`` of ``transformers`` for one sentence: starts from ``[decoder_start_token_id]``, forces the
    target-language token as the first generated token (ForcedBOSTokenLogitsProcessor) and, when ``forced_eos_token_id``
    is given, ``</s>`` as the last allowed one (ForcedEOSTokenLogitsProcessor); stops at ``</s>``.  Returns the ids
    including the start token, as ``generate`` does.  The arg-max runs on the device (``wlk_nllb_topk``): one read-back
    of 8 bytes per token.  Beam search: :func:`beam_search`."""
    cfg = session.model.cfg
    if session.rows != 1:
        raise ValueError("generate: greedy decoding needs a 1-row session")
    eos, start = cfg.eos_token_id, cfg.decoder_start_token_id
    session.encode(src_ids)
    max_length = 1 + max_new_tokens
    out = [start]
    for step in range(max_new_tokens):
        if step == 0:
            session.decode(np.asarray([out], np.int64), first=True)
            best = None
        else:
            best = int(session.step(out[-1:], 1)[1][0, 0])
        cur_len = len(out)
        if forced_bos_token_id is not None and cur_len == 1:
            nxt = int(forced_bos_token_id)
        elif forced_eos_token_id is not None and cur_len == max_length - 1:
            nxt = int(forced_eos_token_id)
        else:
            nxt = best if best is not None else int(session.topk(1)[1][0, 0])
        out.append(nxt)
        if nxt == eos:
            break
    return out


def default_alignment_heads(cfg: NllbConfig) -> List[Tuple[int, int]]:
    """Every head of decoder layer ``decoder_layers // 2``.  A PLACEHOLDER: nobody has validated this choice - or the default
    ``threshold`` of the translation session - on trained weights (no checkpoint exists where this was built); pick heads
    whose arg-max follows the source monotonically on the deployed checkpoint and pass them explicitly."""
    layer = cfg.decoder_layers // 2
    return [(layer, h) for h in range(cfg.attention_heads)]


def generate_alignatt(session, src_ids: Sequence[int], forced_bos_token_id: int, *, committed: Sequence[int] = (),
                      n_accessible: int, threshold: int, final: bool, max_new_tokens: int = 199,
                      device_loop: bool = True) -> Tuple[List[int], List[int], str]:
    """AlignAtt decoding of one update of a streaming sentence -> ``(new ids, their source positions, stop reason)``.

    ``src_ids`` = ``[source language, content..., </s>]`` (S ids); the first ``n_accessible`` of them (language code
    included) belong to committed ASR words, the rest is the unstable tail and ``</s>``.  Decoding continues from
    ``[</s>, forced_bos_token_id, *committed]``: all but the last of these are prefilled, the last and every later token go
    through ``step_align`` (alignment heads must be set) with the content window ``lo = 1``, ``hi = S - 1`` and
    ``limit = max(n_accessible - threshold, lo)``.  Every step yields a candidate ``y`` (the arg-max) and the source
    position ``a`` it leans on:

    * not ``final``: the loop ends WITHOUT emitting ``y`` when ``a < 0`` or ``a >= limit`` (``"attention"``), or when
      ``y`` is ``</s>`` (``"eos"``: an open sentence must not end); otherwise ``y`` is emitted;
    * ``final``: no attention rule; ``</s>`` ends the sentence and is not emitted (``"eos"``);
    * both end after ``max_new_tokens`` (``"length"``) and on a full target context (``"context"``).

    ``device_loop=True`` runs this inside the library (wlk_nllb_generate_alignatt, one call); ``False`` runs the same rule
    here over ``step_align`` - the two agree exactly."""
    cfg = session.model.cfg
    if session.rows != 1:
        raise ValueError("generate_alignatt: needs a 1-row session")
    eos = cfg.eos_token_id
    prompt = [cfg.decoder_start_token_id, int(forced_bos_token_id)] + [int(t) for t in committed]
    S = len(src_ids)
    if not 0 <= n_accessible <= S or threshold < 0 or max_new_tokens < 0:
        raise ValueError("generate_alignatt: needs 0 <= n_accessible <= len(src_ids), threshold >= 0, max_new_tokens >= 0")
    session.encode(src_ids)
    if device_loop:
        return session.generate_alignatt_loop(prompt, n_accessible, threshold, final, eos, max_new_tokens)
    return alignatt_loop(session, prompt, S, n_accessible, threshold, final, eos, max_new_tokens)


def alignatt_loop(session, prompt: Sequence[int], src_len: int, n_accessible: int, threshold: int, final: bool, eos: int,
                  max_new: int) -> Tuple[List[int], List[int], str]:
    """The rule of :func:`generate_alignatt` over ``decode`` + ``step_align`` of an encoded session: wlk_nllb_generate_alignatt
    (csrc/nllb.hip) restated line by line."""
    if len(prompt) < 2:
        raise ValueError("alignatt_loop: the prompt needs at least two tokens (</s>, target language)")
    lo, hi = 1, src_len - 1
    limit = min(max(n_accessible - threshold, lo), src_len)
    max_tgt = getattr(getattr(session.model, "cdims", None), "max_tgt", None)
    session.decode(np.asarray([list(prompt[:-1])], np.int64), first=True)
    fed, last = len(prompt) - 1, int(prompt[-1])
    out: List[int] = []
    align: List[int] = []
    while True:
        if len(out) >= max_new:
            return out, align, "length"
        if max_tgt is not None and fed + 1 > max_tgt:
            return out, align, "context"
        _lp, ids, pos, _prob, _mass = session.step_align([last], 1, lo, hi, limit)
        fed += 1
        y, a = int(ids[0, 0]), int(pos[0])
        if not final and (a < 0 or a >= limit):
            return out, align, "attention"
        if y == eos:
            return out, align, "eos"
        out.append(y)
        align.append(a)
        last = y


def _per_sentence(value, n: int, what: str) -> list:
    if isinstance(value, (list, tuple, np.ndarray)):
        if len(value) != n:
            raise ValueError(f"generate_batch: {what} must be a scalar or one value per sentence")
        return [None if v is None else int(v) for v in value]
    return [None if value is None else int(value)] * n


def clamp_draft(prev_ids: Optional[Sequence[int]], max_new_tokens: int, max_tgt: Optional[int], eos: int) -> List[int]:
    """The draft ``batch.verify`` may be handed for a sentence whose previous result of :func:`generate` was ``prev_ids``
    (``[start, forced, y...]``, possibly ending in ``</s>``): ``prev_ids[2:]`` cut in front of its first ``</s>`` and limited to
    ``min(max_new_tokens - 3, max_tgt - 3)`` tokens (``max_tgt`` ``None``: no context limit) - the token behind an accepted
    draft then lands at output index <= ``max_length - 2``, never where the forced-EOS rule or the length stop decides, and
    ``2 + len(draft) <= max_tgt - 1`` is the prefill's capacity rule.  ``[]`` = no draft."""
    if prev_ids is None:
        return []
    d = [int(t) for t in list(prev_ids)[2:]]
    if eos in d:
        d = d[:d.index(eos)]
    room = int(max_new_tokens) - 3
    if max_tgt is not None:
        room = min(room, int(max_tgt) - 3)
    return d[:room] if room >= 1 else []


def generate_batch(batch, sources: Sequence[Sequence[int]],
                   forced_bos_token_ids: Union[None, int, Sequence[Optional[int]]] = None, *,
                   max_new_tokens: Union[int, Sequence[int]] = 199, forced_eos_token_id: Optional[int] = None,
                   more: Optional[Callable[[], Optional[Iterable[tuple]]]] = None,
                   done: Optional[Callable[[object, List[int]], None]] = None,
                   drafts: Optional[Sequence[Optional[Sequence[int]]]] = None) -> List[List[int]]:
    """Greedy :func:`generate` for any number of sentences through the slots of one batch (``HipNllbBatch``, or anything with
    its ``n_slots`` / ``encode`` / ``step`` / ``release``): ``model.generate`` on a padded batch in ``transformers``, sentence
    by sentence the same ids as :func:`generate` alone.  ``forced_bos_token_ids`` and ``max_new_tokens`` are scalars or one
    value per sentence.

    Sentences are admitted to free slots in order (those admitted together share one stacked encoder pass); every token
    position is ONE ``step`` over the rows still running; a sentence that ends - ``</s>`` or its own length limit -
    releases its slot, and the next waiting sentence is encoded into it and joins at the following step.  The forced-BOS
    and forced-EOS rules are :func:`generate`'s, applied per sentence at that sentence's own length.

    ``more`` is polled once per step (and once more before the pass would end): it may return further
    ``(source, forced_bos, max_new_tokens, ticket)`` work, which queues behind what is already waiting; the ids of such a
    sentence go to ``done(ticket, ids)`` as soon as it ends.  This is how a serving layer joins a running pass.  Returns
    the ids of ``sources`` in input order, each including the start token.

    ``drafts``: one entry (or ``None``) per sentence - a previous result of this sentence's
    translation, e.g. of the same sentence a word shorter; ``more`` may append one as a fifth element.  The sentences admitted
    together that have a usable draft (:func:`clamp_draft`), a forced BOS and a batch with ``verify`` share ONE
    ``batch.verify`` behind their ``encode``: such a sentence starts as ``[start, bos] + draft[:accepted] + [next]`` and joins
    the following ``step`` (or ends there on ``</s>``).  Greedy decoding is a function of the tokens in front of a position,
    so a draft changes how many tokens one pass yields, never which.  A batch without ``verify`` ignores drafts."""
    cfg = batch.model.cfg
    eos, start = cfg.eos_token_id, cfg.decoder_start_token_id
    n = len(sources)
    bos, limits = _per_sentence(forced_bos_token_ids, n, "forced_bos_token_ids"), _per_sentence(max_new_tokens, n, "max_new_tokens")
    if drafts is not None and len(drafts) != n:
        raise ValueError("generate_batch: drafts must hold one entry (or None) per sentence")
    results: List[Optional[List[int]]] = [None] * n
    waiting = [dict(src=sources[i], bos=bos[i], max_new=limits[i], index=i, ticket=None,
                    draft=None if drafts is None else drafts[i]) for i in range(n)]
    free = list(range(batch.n_slots))
    running: Dict[int, dict] = {}                      # slot -> sentence, in admission order
    can_verify = hasattr(batch, "verify")
    max_tgt = getattr(getattr(batch.model, "cdims", None), "max_tgt", None)

    def usable_draft(item) -> List[int]:
        if not can_verify or item.get("draft") is None or item["bos"] is None:
            return []
        d = clamp_draft(item["draft"], item["max_new"], max_tgt, eos)
        for j, t in enumerate(d):                      # what the library would refuse ends the draft, not the pass
            if t < 0 or t >= cfg.vocab_size or t == cfg.pad_token_id:
                return d[:j]
        return d

    def finish(item, slot=None):
        if slot is not None:
            batch.release(slot)
            free.append(slot)
            free.sort()
        if item["index"] is not None:
            results[item["index"]] = item["out"]
        elif done is not None:
            done(item["ticket"], item["out"])

    while True:
        if more is not None:
            for src, fb, mn, ticket, *rest in (more() or ()):
                waiting.append(dict(src=src, bos=None if fb is None else int(fb), max_new=int(mn), index=None, ticket=ticket,
                                    draft=rest[0] if rest else None))
        admitted = []
        while waiting and (free or waiting[0]["max_new"] <= 0):
            item = waiting.pop(0)
            item["out"] = [start]
            if item["max_new"] <= 0:                   # generate's loop does not run: the start token alone
                finish(item)
                continue
            admitted.append((free.pop(0), item))
        if admitted:
            batch.encode([s for s, _ in admitted], [it["src"] for _, it in admitted])
            running.update(admitted)
            drafted = [(s, it, d) for s, it, d in ((s, it, usable_draft(it)) for s, it in admitted) if d]
            if drafted:
                accepted, nxt = batch.verify([s for s, _, _ in drafted], [[start, it["bos"]] + d for _, it, d in drafted])
                for (slot, item, d), k, t in zip(drafted, accepted, nxt):
                    item["out"] = [start, item["bos"]] + d[:int(k)] + [int(t)]
                    if int(t) == eos:                  # (never the length stop: clamp_draft keeps len(out) < max_length)
                        del running[slot]
                        finish(item, slot)
        if not running:
            if waiting:
                continue
            break
        slots = list(running)
        best = batch.step(slots, [running[s]["out"][-1] for s in slots], 1)[1]
        for r, slot in enumerate(slots):
            item = running[slot]
            out = item["out"]
            cur_len, max_length = len(out), 1 + item["max_new"]
            if item["bos"] is not None and cur_len == 1:
                nxt = item["bos"]
            elif forced_eos_token_id is not None and cur_len == max_length - 1:
                nxt = int(forced_eos_token_id)
            else:
                nxt = int(best[r, 0])
            out.append(nxt)
            if nxt == eos or len(out) == max_length:
                del running[slot]
                finish(item, slot)
    return results


def generate_alignatt_batch(batch, requests: Sequence[tuple], *,
                            more: Optional[Callable[[], Optional[Iterable[tuple]]]] = None,
                            done: Optional[Callable[[object, Tuple[List[int], List[int], str]], None]] = None
                            ) -> List[Tuple[List[int], List[int], str]]:
    """:func:`generate_alignatt` for any number of streaming updates through the slots of one batch (``HipNllbBatch`` with
    alignment heads set, or anything with its ``n_slots`` / ``encode`` / ``prefill`` / ``step_align`` / ``release``).  Each
    request is ``(src_ids, forced_bos_token_id, committed, n_accessible, threshold, final, max_new_tokens)`` and is decoded by
    the rule of :func:`alignatt_loop`, unchanged; -> ``(new ids, their source positions, stop reason)`` per request, in input
    order, the same as :func:`generate_alignatt` gives for it alone.

    Admission is :func:`generate_batch`'s: waiting requests take free slots in order; those admitted together share ONE
    stacked ``encode`` and ONE stacked ``prefill`` of their ``prompt[:-1]``; every token position is ONE ``step_align`` over
    the rows still running, each with its own ``lo = 1``, ``hi = S - 1`` and ``limit``; a request that stops (``"attention"``
    before ``"eos"``, ``"length"``, ``"context"``) releases its slot and the next waiting request joins at the following step.
    A request with ``max_new_tokens`` 0 returns ``([], [], "length")`` without taking a slot.

    ``more`` is polled once per step (and once more before the pass would end): it may return further requests with a
    ticket appended, ``(..., max_new_tokens, ticket)``; the outcome of such a request goes to ``done(ticket, outcome)`` as
    soon as it stops.  This is how a serving layer joins a running pass."""
    cfg = batch.model.cfg
    eos, start = cfg.eos_token_id, cfg.decoder_start_token_id
    max_tgt = getattr(getattr(batch.model, "cdims", None), "max_tgt", None)
    results: List[Optional[Tuple[List[int], List[int], str]]] = [None] * len(requests)

    def item_of(req, index, ticket):
        src, bos, committed, n_acc, thr, final, max_new = req
        src = [int(t) for t in src]
        n_acc, thr, max_new = int(n_acc), int(thr), int(max_new)
        if not 0 <= n_acc <= len(src) or thr < 0 or max_new < 0:
            raise ValueError("generate_alignatt_batch: needs 0 <= n_accessible <= len(src_ids), threshold >= 0, max_new_tokens >= 0")
        lo = 1
        return dict(src=src, prompt=[start, int(bos)] + [int(t) for t in committed], lo=lo, hi=len(src) - 1,
                    limit=min(max(n_acc - thr, lo), len(src)), final=bool(final), max_new=max_new, index=index, ticket=ticket,
                    out=[], align=[])

    waiting = [item_of(req, i, None) for i, req in enumerate(requests)]
    free = list(range(batch.n_slots))
    running: Dict[int, dict] = {}                      # slot -> request, in admission order

    def finish(item, why, slot=None):
        if slot is not None:
            del running[slot]
            batch.release(slot)
            free.append(slot)
            free.sort()
        outcome = (item["out"], item["align"], why)
        if item["index"] is not None:
            results[item["index"]] = outcome
        elif done is not None:
            done(item["ticket"], outcome)

    def stopped_before_a_step(item) -> Optional[str]:  # alignatt_loop's checks at the top of its loop
        if len(item["out"]) >= item["max_new"]:
            return "length"
        if max_tgt is not None and item["fed"] + 1 > max_tgt:
            return "context"
        return None

    while True:
        if more is not None:
            for req in (more() or ()):
                waiting.append(item_of(req[:-1], None, req[-1]))
        admitted = []
        while waiting:
            item = waiting[0]
            item["fed"], item["last"] = len(item["prompt"]) - 1, item["prompt"][-1]
            why = stopped_before_a_step(item)
            if why is None and not free:
                break
            waiting.pop(0)
            if why is not None:                        # nothing to decode: no slot is taken
                finish(item, why)
                continue
            admitted.append((free.pop(0), item))
        if admitted:
            slots = [s for s, _ in admitted]
            batch.encode(slots, [it["src"] for _, it in admitted])
            batch.prefill(slots, [it["prompt"][:-1] for _, it in admitted])
            running.update(admitted)
        if not running:
            if waiting:
                continue
            break
        slots = list(running)
        rows = [running[s] for s in slots]
        _lp, ids, pos, _prob, _mass = batch.step_align(slots, [it["last"] for it in rows], 1, [it["lo"] for it in rows],
                                                       [it["hi"] for it in rows], [it["limit"] for it in rows])
        for r, (slot, item) in enumerate(zip(slots, rows)):
            item["fed"] += 1
            y, a = int(ids[r, 0]), int(pos[r])
            if not item["final"] and (a < 0 or a >= item["limit"]):
                finish(item, "attention", slot)
                continue
            if y == eos:
                finish(item, "eos", slot)
                continue
            item["out"].append(y)
            item["align"].append(a)
            item["last"] = y
            why = stopped_before_a_step(item)
            if why is not None:
                finish(item, why, slot)
    return results


def beam_search(session, src_ids: Sequence[int], forced_bos_token_id: Optional[int] = None, *, num_beams: int,
                max_new_tokens: int = 199, length_penalty: float = 1.0, early_stopping=False,
                forced_eos_token_id: Optional[int] = None, device_steps: Optional[bool] = None) -> List[int]:
    """``model.generate(input_ids, forced_bos_token_id=..., num_beams=n, do_sample=False, max_new_tokens=...)`` of
    ``transformers`` 5.x for one sentence (``GenerationMixin._beam_search``, generation/utils.py): per step the 2 n best
    (beam, token) continuations by accumulated log-probability; those among the n best that end (``</s>`` or the length
    limit) compete, with score / generated_length ** length_penalty, for the n finished slots; the n best others run on;
    stop when no running beam can beat the worst finished one (``early_stopping=False``: judged at the current length;
    ``"never"``: at the maximum length when the penalty favours long outputs; ``True``: as soon as n have finished).
    Returns the best finished sequence including the start token.  The device supplies the 2 n best log-probabilities of
    every beam row (``topk``) and reorders the caches (``kv_reorder``); the bookkeeping here is float32 like the original.

    ``device_steps`` (``None``: the environment's ``WLK_NLLB_BEAM_STEPS=1``; only for sessions that have ``step_beam``): the
    prompt is ``decode`` + ``topk(2 n)`` and every later step ONE ``step_beam(tokens, sources of the previous re-ranking,
    2 n)`` - the device's top-16 for any n in 2..8 and the ancestry table instead of ``kv_reorder``; no logits come back and
    no cache row moves.  Everything behind the 2 n candidates is the same code either way."""
    cfg = session.model.cfg
    n, K = int(num_beams), 2 * int(num_beams)
    if n != session.rows:
        raise ValueError(f"beam_search: the session has {session.rows} rows, num_beams = {n}")
    if n > 8:
        raise ValueError("beam_search: at most 8 beams (rows of a session)")
    f32 = np.float32
    V, eos, start, pad = cfg.vocab_size, cfg.eos_token_id, cfg.decoder_start_token_id, cfg.pad_token_id
    prompt_len, cur_len = 1, 1
    max_length = prompt_len + max_new_tokens
    NEG = f32(-1.0e9)
    run_seq = np.full((n, max_length), pad, np.int64)
    run_seq[:, 0] = start
    run_sc = np.full(n, NEG, f32)
    run_sc[0] = 0.0                                  # identical beams at the start: only the first one counts
    fin_seq, fin_sc = run_seq.copy(), np.full(n, NEG, f32)
    fin_done, fin_len = np.zeros(n, bool), np.full(n, prompt_len)
    unsatisfied = True
    if device_steps is None:
        device_steps = os.environ.get("WLK_NLLB_BEAM_STEPS") == "1"
    device_steps = bool(device_steps) and hasattr(session, "step_beam")
    sources = np.arange(n, dtype=np.int32)           # device steps: the rows the running beams continue
    session.encode(src_ids)
    while True:
        if device_steps:
            if cur_len == prompt_len:
                session.decode(run_seq[:, :cur_len], first=True)
                top_lp, top_id = session.topk(K)
            else:
                top_lp, top_id = session.step_beam(run_seq[:, cur_len - 1], sources, K)
            # a row with fewer than K finite logits fills up with (-inf, -1): the padding id keeps such a candidate inside its
            # own row of `flat` below; it ranks last, and were it ever chosen the next step refuses the token
            top_id = np.where(top_id < 0, pad, top_id)
        elif K <= 8:                                  # the device's top-k takes up to 8 per row
            if cur_len == prompt_len:
                session.decode(run_seq[:, :cur_len], first=True)
                top_lp, top_id = session.topk(K)
            else:
                top_lp, top_id = session.step(run_seq[:, cur_len - 1], K)
        else:                                         # 5 .. 8 beams: the rows' logits come back and are cut here
            session.decode(run_seq[:, :cur_len] if cur_len == prompt_len else run_seq[:, cur_len - 1:cur_len],
                           first=(cur_len == prompt_len))
            lp_rows = session.logits().astype(f32)
            lp_rows = lp_rows - _logsumexp(lp_rows)
            top_id = np.argpartition(-lp_rows, K - 1, axis=-1)[:, :K]
            top_lp = np.take_along_axis(lp_rows, top_id, axis=-1)
        forced = None
        if forced_bos_token_id is not None and cur_len == 1:
            forced = int(forced_bos_token_id)
        elif forced_eos_token_id is not None and cur_len == max_length - 1:
            forced = int(forced_eos_token_id)
        if forced is not None:                       # Forced*TokenLogitsProcessor: 0 for the token, -inf for the rest
            top_lp = np.full((n, K), -np.inf, f32)
            top_lp[:, 0] = 0.0
            top_id = np.tile(np.arange(K, dtype=np.int64), (n, 1))
            top_id[top_id == forced] = K               # the filler ids only have to differ from the forced one
            top_id[:, 0] = forced
        total = (top_lp.astype(f32) + run_sc[:, None]).reshape(-1)
        flat = (np.arange(n)[:, None] * V + top_id.astype(np.int64)).reshape(-1)
        order = np.lexsort((flat, -total))[:K]         # descending score, ties by the flattened (beam, token) index
        cand_sc, cand_b, cand_tok = total[order], flat[order] // V, flat[order] % V
        cand_seq = run_seq[cand_b].copy()
        cand_seq[:, cur_len] = cand_tok
        hits = (cand_tok == eos) | (cur_len + 1 >= max_length)
        # the n best continuations that go on
        going = cand_sc + hits.astype(f32) * NEG
        keep = np.argsort(-going, kind="stable")[:n]
        # the finished slots: candidates among the n best that just ended, against what is already there
        ended = hits & (np.arange(K) < n)
        score = (cand_sc / f32((cur_len + 1 - prompt_len) ** length_penalty)).astype(f32)
        score = score + f32(bool(fin_done.all()) and early_stopping is True) * NEG
        score = score + f32(not unsatisfied) * NEG
        score = score + (~ended).astype(f32) * NEG
        all_sc = np.concatenate([fin_sc, score])
        best = np.argsort(-all_sc, kind="stable")[:n]
        fin_seq = np.concatenate([fin_seq, cand_seq])[best]
        fin_done = np.concatenate([fin_done, ended])[best]
        fin_len = np.concatenate([fin_len, np.full(K, cur_len + 1)])[best]
        fin_sc = all_sc[best]
        run_seq, run_sc = cand_seq[keep], going[keep]
        if device_steps:
            sources = cand_b[keep].astype(np.int32)    # handed to the next step_beam; nothing is uploaded after the last step
        else:
            session.kv_reorder(cand_b[keep])
        cur_len += 1
        horizon = (max_length - prompt_len) if (early_stopping == "never" and length_penalty > 0.0) else (cur_len - prompt_len)
        best_running = run_sc[0] / f32(horizon ** length_penalty)
        worst_finished = np.where(fin_done, fin_sc.min(), NEG)
        unsatisfied = unsatisfied and bool((best_running > worst_finished).any())
        if not (unsatisfied and not (bool(fin_done.all()) and early_stopping is True) and not bool(hits.all())):
            break
    return fin_seq[0, :fin_len[0]].tolist()


def _logsumexp(x: np.ndarray) -> np.ndarray:
    m = x.max(axis=-1, keepdims=True)
    return m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True, dtype=np.float32))
