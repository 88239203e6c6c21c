"""Batch `transcribe` with beam search on the device (WLK_TRANSCRIBE_DEVICE_BEAM=1): wlk_pick_topk (csrc/select.hip:
rules_topk_kernel) against the float64 statement of its contract (tests/rules_topk_reference.py), wlk_decode_ancestry
against wlk_kv_reorder + wlk_decode (bitwise), and `decode()` through the device branch against the host branch and the
reference's recorded beam result."""
import numpy as np
import pytest

import helpers as H
from rules_topk_reference import near_ties, rules_mask, rules_topk_reference
from whisperlivekit_amd import _lib, synth, transcribe as TR

pytestmark = pytest.mark.gpu
KAT = H.golden_json("transcribe_kat.json")
_models = {}


def hip_model(name, seed=0):
    from whisperlivekit_amd.engine import HipWhisperModel
    if (name, seed) not in _models:
        assert _lib.load().wlk_device_count() > 0, "no MI355X visible"
        _models[(name, seed)] = HipWhisperModel.synthetic(name, seed)
    return _models[(name, seed)]


@pytest.fixture()
def real_vocab(tmp_path, monkeypatch):
    monkeypatch.setenv("WLK_VOCAB_DIR", H.real_vocab_dir(tmp_path))
    monkeypatch.setenv("WLK_SYNTHETIC_VOCAB", "0")


# ---- the kernel against float64 -----------------------------------------------------------------------------------------
ROW_HISTORIES = [                      # per row count: sampled histories of one length, cycled over the rows
    lambda tb, t: [[tb, t[0], tb + 40, tb + 40], [tb, t[1], t[2], tb + 77], [tb, t[3], t[4], t[5]], [t[6], t[7], t[8], t[9]],
                   [tb, tb, t[10], t[11]], [tb, t[12], t[13], tb + 1499], [tb, t[14], tb + 700, tb + 700]],
]


def kernel_cases(dec, rows, rng):
    """(tokens the rows are prefilled with, tokens the rule state is read from) - rows with different histories side by
    side, among them a closed pair (ts_mode 1) beside an opening timestamp (ts_mode 2) with another bound; the first step
    (every row is the prompt) over logits of rows that differ in their last token."""
    tb = dec.tok.timestamp_begin
    t = [int(x) for x in rng.integers(300, 20000, 16)]
    hist = ROW_HISTORIES[0](tb, t)
    mixed = np.asarray([list(dec.initial) + hist[r % len(hist)] for r in range(rows)], np.int64)
    prompt = np.asarray([list(dec.initial)] * rows, np.int64)
    differing = np.concatenate([prompt, rng.integers(300, 20000, (rows, 1))], axis=1)
    one = np.asarray([list(dec.initial) + ([tb + 3] if r % 2 else [tb]) for r in range(rows)], np.int64)
    return [(mixed, mixed), (differing, prompt), (one, one)]


KERNEL_OPTIONS = [dict(), dict(without_timestamps=True), dict(suppress_blank=False, suppress_tokens=""),
                  dict(max_initial_timestamp=None)]


def kernel_sweep(model, rows, session, name):
    """Every (options, case) of one model and row count -> (entries compared, entries left out as float64 near-ties, worst
    error of the device against float64, worst error of the host fp32 rules against float64).  `session` needs decode,
    export, set_rules and pick_topk; without pick_topk (the CPU check of the seeds) only the near-ties are counted."""
    V = model.dims.n_vocab
    rng = np.random.default_rng(1000 + rows)
    n_cmp = n_out = 0
    err_dev = err_host = 0.0
    k = rows + 1
    for options in KERNEL_OPTIONS:
        dec = TR._WindowDecoder(model, TR.DecodingOptions(language="en", temperature=0.0, beam_size=rows, **options))
        mask = rules_mask(V, dec.suppressed or [], dec.blank_ids or [])
        if hasattr(session, "pick_topk"):
            session.set_rules(dec.suppressed or [], dec.blank_ids or [])
        for fed, described in kernel_cases(dec, rows, rng):
            session.decode(fed, first=True, sot_index=dec.sot_index)
            logits = TR._logits(session, rows, V).copy()
            states = dec._pick_states(described)
            if rows >= 2 and fed is described and fed.shape[1] - dec.sample_begin == 4 and not options.get("without_timestamps"):
                assert (states[0]["ts_mode"], states[1]["ts_mode"]) == (1, 2) and states[0]["ts_bound"] != states[1]["ts_bound"]
            want_lp, want_id = rules_topk_reference(logits, mask, states, k)
            sure = ~near_ties(logits, mask, states, k)
            n_cmp += sure.size
            n_out += int((~sure).sum())
            if not hasattr(session, "pick_topk"):
                continue
            got_lp, got_id = session.pick_topk(states, k)
            assert got_lp.shape == got_id.shape == (rows, k)
            assert np.array_equal(got_id[sure], want_id[sure]), (name, rows, options, got_id.tolist(), want_id.tolist())
            host = dec._apply_rules(logits.copy(), described)                # fp32 log_softmax under the host rules
            fin = sure & (want_id >= 0)
            host_at = np.take_along_axis(host, np.maximum(want_id, 0).astype(np.int64), axis=1)
            err_dev = max(err_dev, float(np.abs(got_lp[fin] - want_lp[fin]).max()))
            err_host = max(err_host, float(np.abs(host_at[fin] - want_lp[fin]).max()))
            assert np.isneginf(got_lp[sure & (want_id < 0)]).all()
    return n_cmp, n_out, err_dev, err_host


def encoded_session(model, rows, seconds=3.0, seed=5, debug=False):
    s = model.new_session(beam=rows, max_audio_seconds=1.0, batched=False)
    if debug:
        s.set_debug(True)
    s.encode_mel(TR.pad_or_trim(s.log_mel(synth.speech_like(seconds, seed=seed))))
    return s


@pytest.mark.parametrize("rows", [2, 5, 7])
@pytest.mark.parametrize("name", ["micro.en", "micro"])
def test_pick_topk_against_float64(name, rows, real_vocab):
    """Ids equal, log-probability error against float64 at most twice that of the host fp32 rules on the same cases (the
    summation orders differ: 1024-way strided + butterfly against numpy's pairwise sum).  Left out: entries where float64
    itself is within 1e-4 of a tie (ranking or timestamps-versus-text), at most 2 % of them."""
    model = hip_model(name)
    assert model.dims.n_vocab % 1024 != 0                       # the strided tail is in play
    s = encoded_session(model, rows)
    try:
        n_cmp, n_out, err_dev, err_host = kernel_sweep(model, rows, s, name)
    finally:
        s.close()
    print(f"[transcribe beam] pick_topk {name} rows {rows}: {n_cmp} entries, {n_out} near-ties left out, "
          f"device error {err_dev:.3e}, host fp32 error {err_host:.3e}")
    assert n_cmp >= 12 * rows * (rows + 1) and n_out <= 0.02 * n_cmp, (n_cmp, n_out)
    assert err_dev <= 2 * err_host, (err_dev, err_host)


def test_a_row_that_allows_fewer_than_k_entries(real_vocab):
    model = hip_model("micro.en")
    V = model.dims.n_vocab
    dec = TR._WindowDecoder(model, TR.DecodingOptions(language="en", temperature=0.0, beam_size=2))
    s = encoded_session(model, 2)
    try:
        s.set_rules(dec.suppressed or [], dec.blank_ids or [])
        tokens = np.asarray([list(dec.initial) + [400], list(dec.initial) + [500]], np.int64)
        s.decode(tokens, first=True, sot_index=dec.sot_index)
        logits = TR._logits(s, 2, V).copy()
        full = dec._pick_states(tokens)[0]
        # behind an opening timestamp with the text / timestamp border three ids below the end: three entries are left
        short = dict(full, timestamp_begin=V - 3, eot=V - 3, ts_mode=2, ts_bound=V - 3, no_timestamps=-1)
        mask = rules_mask(V, dec.suppressed or [], dec.blank_ids or [])
        got_lp, got_id = s.pick_topk([short, full], 8)
        want_lp, want_id = rules_topk_reference(logits, mask, [short, full], 8)
        assert sorted(want_id[0, :3].tolist()) == [V - 3, V - 2, V - 1] and (want_id[0, 3:] == -1).all()
        sure = ~near_ties(logits, mask, [short, full], 8)
        assert sure[0].all() and np.array_equal(got_id[sure], want_id[sure])
        assert np.isneginf(got_lp[0, 3:]).all() and np.isfinite(got_lp[0, :3]).all() and np.isfinite(got_lp[1]).all()
        assert np.abs(got_lp[0, :3] - want_lp[0, :3]).max() <= 1e-5
        assert float(np.exp(got_lp[0, :3].astype(np.float64)).sum()) == pytest.approx(1.0, abs=1e-5)
    finally:
        s.close()


def test_argument_checks(real_vocab):
    model = hip_model("micro.en")
    dec = TR._WindowDecoder(model, TR.DecodingOptions(language="en", temperature=0.0, beam_size=2))
    s = encoded_session(model, 2)
    try:
        tokens = np.asarray([list(dec.initial)] * 2, np.int64)
        states = dec._pick_states(tokens)
        s.decode(tokens, first=True, sot_index=dec.sot_index)
        with pytest.raises(_lib.WlkError, match="error -3"):             # WLK_ERR_STATE: no rule set yet
            s.pick_topk(states, 3)
        s.set_rules(dec.suppressed or [], dec.blank_ids or [])
        with pytest.raises(_lib.WlkError, match="error -1"):             # WLK_ERR_ARG
            s.pick_topk(states, 9)
        with pytest.raises(_lib.WlkError, match="error -1"):
            s.pick_topk(states[:1], 3)
        lp, ids = s.pick_topk(states, 3)
        assert np.isfinite(lp).all() and (ids >= dec.tok.timestamp_begin).all()      # a window opens with a timestamp
    finally:
        s.close()
    fresh = model.new_session(beam=2, max_audio_seconds=1.0, batched=False)
    try:
        fresh.set_rules(dec.suppressed or [], dec.blank_ids or [])
        with pytest.raises(_lib.WlkError, match="error -3"):             # WLK_ERR_STATE: nothing decoded yet
            fresh.pick_topk(states, 3)
    finally:
        fresh.close()


# ---- the ancestry step through the public call ---------------------------------------------------------------------------
def test_decode_ancestry_equals_reorder_and_decode_bitwise():
    """tiny.en, 5 rows, 8 steps with shared and dropped ancestors, then the same after a new prefill: logits_last of
    wlk_decode_ancestry bitwise equal to wlk_kv_reorder + wlk_decode after every step, and the state rule of the table."""
    beam = 5
    model = hip_model("tiny.en")
    V = model.dims.n_vocab
    rng = np.random.default_rng(beam)
    prompt = np.tile(np.array([[50257, 50362] + rng.integers(300, 40000, 5).tolist()], np.int64), (beam, 1))
    ref, anc = (encoded_session(model, beam) for _ in range(2))
    try:
        for infer in range(2):                            # the second infer: a prefill that follows an ancestry infer
            for sess in (ref, anc):
                sess.decode(prompt, first=True, sot_index=0)
            for step in range(8):
                if step == 0:
                    src = np.arange(beam)
                elif step == 1:
                    src = np.full(beam, rng.integers(0, beam))            # one ancestor shared by all, the rest dropped
                else:
                    src = np.sort(rng.integers(0, beam, beam))[::(-1 if step % 2 else 1)].copy()
                tokens = rng.integers(300, 40000, (beam, 1)).astype(np.int64)
                ref.kv_reorder(src.tolist())
                ref.decode(tokens, first=False)
                anc.decode_ancestry(tokens[:, 0], src)
                want = ref.export("logits_last", beam * V).view(np.uint32)
                got = anc.export("logits_last", beam * V).view(np.uint32)
                assert (want == got).all(), (infer, step, src.tolist(), int((want != got).sum()))
            assert anc.beam_stats()["ancestry_steps"] == 8 * (infer + 1) and ref.beam_stats()["ancestry_steps"] == 0
            with pytest.raises(_lib.WlkError, match="error -3"):         # the cache rows are not the hypotheses any more
                anc.kv_reorder(list(range(beam))[::-1])
            with pytest.raises(_lib.WlkError, match="error -3"):
                anc.decode(prompt[:, :1], first=False)
    finally:
        ref.close()
        anc.close()


def test_decode_ancestry_of_a_debug_session_is_reorder_and_decode():
    """A session that does not qualify (debug) makes the two calls inside the library: the logits of a debug session that
    makes them itself, bitwise, and no ancestry steps."""
    beam = 3
    model = hip_model("tiny.en")
    V = model.dims.n_vocab
    rng = np.random.default_rng(9)
    prompt = np.tile(np.array([[50257, 50362, 700, 800]], np.int64), (beam, 1))
    ref, dbg = (encoded_session(model, beam, debug=True) for _ in range(2))
    try:
        for sess in (ref, dbg):
            sess.decode(prompt, first=True, sot_index=0)
        for src in ([0, 0, 2], [2, 1, 1], [1, 2, 0]):
            tokens = rng.integers(300, 40000, (beam, 1)).astype(np.int64)
            ref.kv_reorder(src)
            ref.decode(tokens, first=False)
            dbg.decode_ancestry(tokens[:, 0], src)
            want = ref.export("logits_last", beam * V).view(np.uint32)
            got = dbg.export("logits_last", beam * V).view(np.uint32)
            assert (want == got).all(), src
        assert dbg.beam_stats()["ancestry_steps"] == 0
    finally:
        ref.close()
        dbg.close()


# ---- end to end ------------------------------------------------------------------------------------------------------
def window_of(model, audio):
    s = TR._rows_of(model).get(1)
    mel = s.log_mel(audio, padding=TR.N_SAMPLES)
    return TR.pad_or_trim(mel[:, :min(TR.N_FRAMES, mel.shape[-1] - TR.N_FRAMES)])


def both_paths(model, window, monkeypatch, rows, **opts):
    monkeypatch.setenv("WLK_TRANSCRIBE_DEVICE_BEAM", "0")
    host = TR.decode(model, window, **opts)
    sess = TR._rows_of(model).get(rows)
    before = sess.beam_stats()["ancestry_steps"]
    monkeypatch.setenv("WLK_TRANSCRIBE_DEVICE_BEAM", "1")
    dev = TR.decode(model, window, **opts)
    return host, dev, sess.beam_stats()["ancestry_steps"] - before


def test_decode_with_the_device_beam_gives_the_recorded_result(real_vocab, monkeypatch):
    case = next(c for c in KAT if c["name"] == "beam_then_best_of")
    kw, spec = case["kwargs"], case["audio"]
    assert case["calls"][0]["beam"] == 3 and kw["patience"] == 1.5
    model = hip_model(case["model"])
    try:
        window = window_of(model, synth.white_noise(spec["seconds"], seed=spec["seed"]))
        host, dev, anc_steps = both_paths(model, window, monkeypatch, 3, language=kw["language"], temperature=0.0, beam_size=3,
                                          patience=1.5, length_penalty=kw["length_penalty"])
        assert dev.tokens == case["calls"][0]["result"]["tokens"]
        assert dev.tokens == host.tokens
        assert dev.avg_logprob == pytest.approx(host.avg_logprob, abs=1e-4)
        assert dev.avg_logprob == pytest.approx(case["calls"][0]["result"]["avg_logprob"], abs=5e-4)
        assert dev.no_speech_prob == pytest.approx(host.no_speech_prob, rel=1e-5)
        assert anc_steps > 0
    finally:
        TR.release_sessions(model)


def test_decode_beam5_on_tiny_device_path_equals_host_path(real_vocab, monkeypatch):
    model = hip_model("tiny.en")
    try:
        # seeded weights end a window after a few tokens; patience 2 keeps the search going to the length limit, so the
        # two paths are compared over 47 single-token steps with re-ranked hypotheses
        window = window_of(model, synth.white_noise(7.0, seed=13))
        host, dev, anc_steps = both_paths(model, window, monkeypatch, 5, language="en", temperature=0.0, beam_size=5,
                                          patience=2.0, sample_len=48)
        print(f"[transcribe beam] tiny.en beam 5: {len(dev.tokens)} tokens, {anc_steps} ancestry steps, "
              f"avg_logprob device {dev.avg_logprob:.6f} host {host.avg_logprob:.6f}")
        assert dev.tokens == host.tokens
        assert dev.avg_logprob == pytest.approx(host.avg_logprob, abs=1e-4)
        assert anc_steps == 47                            # every single-token step ran over the ancestry table
    finally:
        TR.release_sessions(model)
