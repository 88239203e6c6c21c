"""CPU stand-in for the alignment surface of HipNllbSession (set_alignment_heads / step_align / alignment / align_stats):
an OracleNllbSession whose single-token step is restated here, with the oracle's helpers, so that the selected heads'
cross-attention rows are at hand.  Test infrastructure only.

The read-out restates the library's order (include/wlk_hip.h, wlk_nllb_step_align): the heads' float32 rows are added in
rank order, the sum is multiplied by float32(1 / n), the arg-max of [lo, hi) takes the lowest position of equal values and
is -1 for an empty window, the mass is the sum from `limit` on.  Pinned by tests/golden/nllb_align_kat.npz
(tests/test_nllb_alignatt.py)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.nllb_oracle import OracleNllbSession, _heads, _lin, _ln

GAIN = 8.0        # scripts/gen_golden_nllb_align.py


def align_gain_state_dict(cfg, seed, gain=GAIN):
    """the weights of the fixture: synth_state_dict with every decoder layer's encoder_attn.q_proj multiplied by `gain`"""
    from whisperlivekit_amd import nllb
    sd = nllb.synth_state_dict(cfg, seed)
    for i in range(cfg.decoder_layers):
        for leaf in ("weight", "bias"):
            name = f"model.decoder.layers.{i}.encoder_attn.q_proj.{leaf}"
            sd[name] = (sd[name] * np.float32(gain)).astype(np.float32)
    return sd


def readout(probs, lo, hi, limit):
    """probs [n_align][rows][S] float32 -> (p [rows][S] float32, pos [rows], prob [rows], mass [rows])"""
    probs = np.asarray(probs, np.float32)
    n, rows, S = probs.shape
    p = np.zeros((rows, S), np.float32)
    for a in range(n):
        p = p + probs[a]
    p = p * np.float32(1.0 / n)
    lo, hi = max(lo, 0), min(hi, S)
    pos = np.full(rows, -1, np.int32)
    prob = np.zeros(rows, np.float32)
    for r in range(rows):
        if hi > lo:
            pos[r] = lo + int(np.argmax(p[r, lo:hi]))
            prob[r] = p[r, pos[r]]
    return p, pos, prob, p[:, limit:].sum(axis=1, dtype=np.float32)


def _attend_probs(q, k, v, n_head):
    """oracle.nllb_oracle._attend without a mask, returning the probabilities too"""
    qh, kh, vh = _heads(q, n_head), _heads(k, n_head), _heads(v, n_head)
    w = F.softmax(torch.matmul(qh, kh.transpose(-1, -2)) * (qh.shape[-1] ** -0.5), dim=-1)
    o = torch.matmul(w, vh).transpose(-3, -2)
    return o.reshape(*o.shape[:-2], -1), w


class AlignOracleNllbSession(OracleNllbSession):
    def __init__(self, oracle, rows=1):
        super().__init__(oracle, rows)
        self.heads, self._p = [], None
        self.n_align_steps = 0

    def set_alignment_heads(self, pairs):
        pairs = [(int(l), int(h)) for l, h in pairs]
        cfg = self.oracle.cfg
        if len(pairs) > 64 or len(set(pairs)) != len(pairs) or any(
                not (0 <= l < cfg.decoder_layers and 0 <= h < cfg.attention_heads) for l, h in pairs):
            raise ValueError("bad alignment heads")
        self.heads = pairs

    def encode(self, src_ids):
        super().encode(src_ids)
        self._p = None

    @torch.no_grad()
    def _step_with_attention(self, tokens):
        """NllbOracle.decode for ONE token per row on top of the cache (no causal mask needed), keeping cross-attention"""
        o, cfg, sd, cache, enc = self.oracle, self.oracle.cfg, self.oracle.sd, self.cache, self.enc
        past = cache["k"][0].shape[1]
        x = o._embed(tokens, past)
        kept = {}
        for i in range(cfg.decoder_layers):
            p = f"model.decoder.layers.{i}."
            h = _ln(x, sd, p + "self_attn_layer_norm")
            k = torch.cat([cache["k"][i], _lin(h, sd, p + "self_attn.k_proj")], dim=1)
            v = torch.cat([cache["v"][i], _lin(h, sd, p + "self_attn.v_proj")], dim=1)
            cache["k"][i], cache["v"][i] = k, v
            a, _ = _attend_probs(_lin(h, sd, p + "self_attn.q_proj"), k, v, cfg.attention_heads)
            x = x + _lin(a, sd, p + "self_attn.out_proj")
            h = _ln(x, sd, p + "encoder_attn_layer_norm")
            a, w = _attend_probs(_lin(h, sd, p + "encoder_attn.q_proj"), cache["xk"][i], cache["xv"][i], cfg.attention_heads)
            kept[i] = w[:, :, 0, :]                                        # [rows, H, S]
            x = x + _lin(a, sd, p + "encoder_attn.out_proj")
            h = _ln(x, sd, p + "final_layer_norm")
            x = x + _lin(F.relu(_lin(h, sd, p + "fc1")), sd, p + "fc2")
        x = _ln(x, sd, "model.decoder.layer_norm")
        return F.linear(x, o.emb)[:, -1], kept

    def step_align(self, tokens, k, lo, hi, limit):
        if not self.heads:
            raise RuntimeError("step_align before set_alignment_heads")
        t = torch.as_tensor(np.asarray(tokens), dtype=torch.int64).view(-1, 1)
        self.last, kept = self._step_with_attention(t)
        probs = np.stack([kept[l][:, h, :].numpy() for l, h in self.heads])       # [n_align][rows][S]
        self._p, pos, prob, mass = readout(probs, lo, hi, limit)
        self.n_align_steps += 1
        lp, ids = self.topk(k)
        return lp, ids, pos, prob, mass

    def alignment(self):
        return self._p.copy()

    def align_stats(self):
        return {"align_steps": self.n_align_steps, "graph_captures": 0}

    def close(self):
        pass


class AlignOracleModel:
    """What HipNllbTranslationModel needs from a HipNllbModel, answered by the stand-in."""

    def __init__(self, oracle):
        self.cfg, self.oracle = oracle.cfg, oracle

    def new_session(self, rows=1):
        return AlignOracleNllbSession(self.oracle, rows)


# ---- the fixture (tests/golden/nllb_align_kat.npz) ---------------------------------------------------------------------
REASONS = ("attention", "eos", "length", "context")


def settings_of(kat, prefix):
    """-> [(k, n_accessible, threshold, final, committed ids, max_new, want ids, want alignments, want reason)]"""
    greedy = kat[prefix + "greedy"].tolist()
    out = []
    for k, (n_acc, thr, final, c, max_new) in enumerate(kat[prefix + "settings"].tolist()):
        out.append((k, n_acc, thr, bool(final), greedy[:c], max_new, kat[f"{prefix}out_ids{k}"].tolist(),
                    kat[f"{prefix}out_align{k}"].tolist(), REASONS[int(kat[prefix + "reasons"][k])]))
    return out


def follow_greedy(sess, kat, prefix, atol, min_gap=0.0):
    """Feeds the stored greedy tokens through step_align (content window, limit 0): p within `atol` of the float64 model's,
    the position identical wherever the stored gap exceeds `min_gap`, the candidate the stored one.  -> largest |p - p64|"""
    src, lang, greedy = kat[prefix + "src"], int(kat[prefix + "lang"]), kat[prefix + "greedy"].tolist()
    S = len(src)
    sess.encode(src)
    sess.decode(np.asarray([[sess.model.cfg.decoder_start_token_id]], np.int64), first=True)
    worst = 0.0
    for t, tok in enumerate([lang] + greedy[:-1]):
        _lp, ids, pos, prob, mass = sess.step_align([tok], 1, 1, S - 1, 0)
        p = sess.alignment()
        assert p.shape == (1, S)
        want = kat[prefix + "p64"][t]
        worst = max(worst, float(np.abs(p[0] - want).max()))
        np.testing.assert_allclose(p[0], want, rtol=0, atol=atol, err_msg=f"step {t}")
        if kat[prefix + "gap"][t] > min_gap:
            assert int(pos[0]) == int(kat[prefix + "pos"][t]), f"step {t}"
            assert abs(float(prob[0]) - want[int(pos[0])]) <= atol
        assert int(ids[0, 0]) == greedy[t], f"step {t}"
        assert abs(float(mass[0]) - want.sum()) <= atol
    return worst


# ---- a 12-word sentence through both streaming policies (CPU over the stand-in, GPU over the library) -------------------
SENTENCE = "the quick brown fox jumps over the lazy dog near the river."


class HypothesisTail:
    """the unstable ASR tail as the audio processor queues it (translation sessions match it by class name)"""

    def __init__(self, text):
        self.text, self.start, self.end = text, None, None


class CountingSession:
    """a session that counts the single-token decoder steps it is asked for"""

    def __init__(self, sess):
        self._s, self.steps = sess, 0

    def __getattr__(self, name):
        return getattr(self._s, name)

    def step(self, *a, **kw):
        self.steps += 1
        return self._s.step(*a, **kw)


def stream_twelve_words(model, tokenizer, words, max_new_tokens=24, threshold=2):
    """SENTENCE arrives word by word with a two-word hypothesis tail, under both policies.  Checks that the AlignAtt text is
    append-only and that its final is generate_alignatt(final=True) from the committed prefix; -> (AlignAtt decoder steps,
    local-agreement decoder steps, report line)."""
    from whisperlivekit_amd import nllb
    from whisperlivekit_amd import translation as T
    toks = words(SENTENCE)
    assert len(toks) == 12
    tm = T.HipNllbTranslationModel(model, tokenizer, policy="alignatt", threshold=threshold, hypothesis_tail=True,
                                   max_new_tokens=max_new_tokens)
    now = [0.0]
    tr = tm.new_session("eng_Latn", "fra_Latn")
    tr._clock = lambda: now[0]
    local = T.HipNllbTranslationModel(model, tokenizer, max_new_tokens=max_new_tokens).new_session("eng_Latn", "fra_Latn")
    local.session = CountingSession(local.session)
    check = model.new_session(1)
    try:
        assert isinstance(tr, T.HipAlignAttTranslation) and type(local) is T.HipOnlineTranslation
        shown = ""
        for i, w in enumerate(toks[:-1]):
            now[0] += 1.0
            tr.insert_tokens([w, HypothesisTail(" ".join(t.text.strip() for t in toks[i + 1:i + 3]))])
            new, buf = tr.process()
            assert new is None and (buf.text or "").startswith(shown), (i, shown, buf.text)
            shown = buf.text or ""
            local.insert_tokens([w])
            local.process()
        now[0] += 1.0
        tr.insert_tokens([HypothesisTail(toks[-1].text.strip() + " and")])          # a tail-only update
        new, buf = tr.process()
        assert new is None and (buf.text or "").startswith(shown)
        shown = buf.text or ""
        committed = list(tr._open.ids)
        assert tm.decode(committed).strip() == shown
        tr.insert_tokens(toks[-1:])
        local.insert_tokens(toks[-1:])
        new, buf = tr.process()
        local.process()
        # the final pass = generate_alignatt(final=True) from the same committed prefix
        src = tm.encode(" ".join(t.text.strip() for t in toks), "eng_Latn")
        check.set_alignment_heads(nllb.default_alignment_heads(model.cfg))
        more, _, why = nllb.generate_alignatt(check, src, tr.target_id, committed=committed, n_accessible=len(src),
                                              threshold=threshold, final=True, max_new_tokens=max_new_tokens - len(committed),
                                              device_loop=hasattr(check, "generate_alignatt_loop"))
        assert isinstance(new, T.Translation) and new.text == tm.decode(committed + more).strip() and new.text.startswith(shown)
        assert (new.start, new.end) == (0.0, toks[-1].end) and not buf.text
        align_steps = tr.session.align_stats()["align_steps"]
        report = (f"12 words: AlignAtt {align_steps} decoder steps in {tr.updates} updates + {tr.finals} final (the final ended on "
                  f"{why}; {len(committed)} tokens were committed before it), local agreement {local.session.steps} steps in "
                  f"{local.translations} translations")
        return align_steps, local.session.steps, report
    finally:
        tr.close(); local.close(); check.close()
