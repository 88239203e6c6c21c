"""TEST INFRASTRUCTURE: what `whisperlivekit_amd.nllb.generate_batch` and the serving glue call on a `HipNllbBatch`,
answered per slot by the CPU oracle (oracle/nllb_oracle.py NllbOracle).  Every slot is an independent one-sentence
decoder, so whatever the host loop does with slots - admission order, refill, release - must reproduce the
single-sentence results.  The contract errors of the library (csrc/nllb_batch.hip) are restated so that the host loop is
tested against them too."""
import types

import numpy as np
import torch


class OracleNllbBatch:
    def __init__(self, oracle, n_slots=8, on_step=None):
        if not 1 <= n_slots <= 8:
            raise ValueError("1..8 slots")
        self.oracle, self.n_slots = oracle, n_slots
        self.model = types.SimpleNamespace(cfg=oracle.cfg)
        self.enc = [None] * n_slots
        self.cache = [None] * n_slots
        self.last = [None] * n_slots
        self.on_step = on_step                   # hook(batch, slots): tests inject a failure or a rendezvous here
        self.n_steps = self.n_rows = self.n_encodes = 0
        self.closed = False

    def _check(self, slots):
        slots = [int(s) for s in slots]
        if len(set(slots)) != len(slots):
            raise ValueError("a slot is named twice in one call")
        if not slots or any(s < 0 or s >= self.n_slots for s in slots):
            raise ValueError("slot index out of range")
        return slots

    def encode(self, slots, sources):
        slots = self._check(slots)
        assert len(slots) == len(sources)
        for s, src in zip(slots, sources):
            self.enc[s] = self.oracle.encode([int(t) for t in src])
            self.cache[s] = self.oracle.new_cache()
            self.last[s] = None
        self.n_encodes += 1

    def step(self, slots, tokens, k=1):
        slots = self._check(slots)
        assert len(slots) == len(tokens)
        if any(self.enc[s] is None for s in slots):
            raise RuntimeError("step on a slot that is not encoded")
        if self.on_step is not None:
            self.on_step(self, slots)
        lp = np.empty((len(slots), k), np.float32)
        ids = np.empty((len(slots), k), np.int32)
        for r, (s, tok) in enumerate(zip(slots, tokens)):
            self.last[s] = self.oracle.decode(torch.tensor([[int(tok)]]), self.enc[s], self.cache[s])[0, -1]
            v, i = torch.log_softmax(self.last[s], dim=-1).topk(k)
            lp[r], ids[r] = v.numpy(), i.numpy()
        self.n_steps += 1
        self.n_rows += len(slots)
        return lp, ids

    def release(self, slot):
        self._check([slot])
        self.enc[slot] = self.cache[slot] = self.last[slot] = None

    def encoder_output(self, slot):
        return self.enc[slot].numpy()

    def logits(self, slot):
        return self.last[slot].numpy().copy()

    def close(self):
        self.closed = True
