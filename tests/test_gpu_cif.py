"""CIF end-of-word head on the device: the two kernels of csrc/cif.hip against the reference's recorded
answers and a float64 evaluation (tests/cif_reference.py), stacked against solo, and the opt-in switch end to end.

The contract under test: the device gives the reference's answer wherever float64 decides the case with the margin R
of the fixture; alphas stay inside the worst-case rounding bound of an fp32 dot product; a session's alphas and record
have the same bits alone and stacked; the X3 input form gives the bits of the fp32 form.

Measured on MI355X (804 cases + the 252 d = 1280 cases again from the X3 image): 780 decided evaluations, none wrong;
largest |alpha - alpha64| / bound = 0.0094."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import cif_reference as cr
import helpers as H

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(H.GOLDEN, "cif_device_kat.npz")
CKPT = os.path.join(H.GOLDEN, "cif_micro.pt")
WLK_ERR_ARG, WLK_ERR_STATE = -1, -3


def diag_cif(blocks, w, bias, as_x3=False, t_each=None):
    """wlk_diag_cif: blocks = list of [T_i, d] fp32 arrays (one stacked launch) -> [(alphas [T_i], record dict)]"""
    from whisperlivekit_amd import _lib
    lib = _lib.load()
    n = len(blocks)
    T = max(b.shape[0] for b in blocks)
    d = blocks[0].shape[1]
    feat = np.zeros((n, T, d), np.float32)
    for i, b in enumerate(blocks):
        feat[i, : b.shape[0]] = b
    te = np.asarray([b.shape[0] for b in blocks], np.int32) if t_each is None else np.asarray(t_each, np.int32)
    alphas = np.full((n, T), np.nan, np.float32)
    out = (_lib.CifOut * n)()
    w = np.ascontiguousarray(w, np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    _lib.check(lib.wlk_diag_cif(vp(feat), T, d, vp(w), float(bias), 1 if as_x3 else 0, n, vp(te), vp(alphas),
                                C.cast(out, C.c_void_p)))
    fields = [f[0] for f in _lib.CifOut._fields_]
    return [(alphas[i, : te[i]].copy(), {f: getattr(out[i], f) for f in fields}) for i in range(n)]


def kat_cases():
    import torch
    ck = torch.load(CKPT, map_location="cpu", weights_only=True)
    w, b = ck["weight"].float().numpy().reshape(-1), float(ck["bias"].reshape(-1)[0])
    R = cr.load_fixture(FIXTURE)["R"]
    for k in H.golden_json("cif_kat.json"):
        x = cr.kat_features(k)
        yield dict(d=128, T=k["T"], kind="kat", scale=k["scale"], seed=k["seed"], fire=k["fire"]), x, cr.evaluate(x, w, b, R), w, b


_RUN = {}


def device_run():
    """Every fixture case and every cif_kat.json case through the kernels, once per process:
    -> list of dict(case, ev, alpha, rec, bound, alpha_x3, rec_x3)."""
    if "rows" in _RUN:
        return _RUN["rows"]
    fx = cr.load_fixture(FIXTURE)
    rows = []

    def one(c, x, ev, w, b):
        alpha, rec = diag_cif([x], w, b)[0]
        row = dict(case=c, ev=ev, alpha=alpha, rec=rec, bound=cr.alpha_bound(x, w), alpha_x3=None, rec_x3=None)
        if c["d"] == 1280:
            row["alpha_x3"], row["rec_x3"] = diag_cif([x], w, b, as_x3=True)[0]
        rows.append(row)

    for c, x, ev in cr.iter_fixture(FIXTURE):
        one(c, x, ev, *fx["heads"][c["d"]])
    for c, x, ev, w, b in kat_cases():
        one(c, x, ev, w, b)
    _RUN["rows"] = rows
    return rows


def test_decisions_match_the_reference_on_every_decided_case():
    rows = device_run()
    decided = wrong = 0
    report = []
    for r in rows:
        c, ev = r["case"], r["ev"]
        for rec in (r["rec"], r["rec_x3"]):
            if rec is None:
                continue
            assert rec["seq"] == 1
            if not ev["decided"]:
                continue
            decided += 1
            got = (bool(rec["fire"]), rec["n"], rec["cnt"], rec["pos"])
            want = (c["fire"], ev["n"], ev["cnt"], ev["pos"])
            if got != want or ev["fire"] != c["fire"]:
                wrong += 1
                report.append((c, got, want))
    print(f"decided evaluations: {decided}, wrong: {wrong}")
    assert wrong == 0, report[:5]
    assert decided >= 0.6 * len(rows)


def test_resize_loop_rounds_match_float64_on_decided_cases():
    rows = [r for r in device_run() if r["ev"]["decided"]]
    entered = [r for r in rows if r["ev"]["resize_rounds"] > 0]
    assert len(entered) >= 20
    for r in rows:
        assert r["rec"]["resize_rounds"] == r["ev"]["resize_rounds"], (r["case"], r["rec"], r["ev"]["resize_rounds"])
        # without the loop the answer is integ[T-3] < cnt <= integ[T-2] (diagnostic cross-check of the record)
        if r["ev"]["resize_rounds"] == 0:
            assert bool(r["rec"]["fire"]) == cr.no_resize_cross_check(r["ev"], r["case"]["T"])


def test_alphas_within_the_derived_bound_of_float64():
    worst = 0.0
    for r in device_run():
        err = np.abs(r["alpha"].astype(np.float64) - r["ev"]["alpha"])
        ratio = float((err / r["bound"]).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (r["case"], ratio)
    print(f"largest |alpha - alpha64| / bound: {worst:.4f}")


def test_x3_input_gives_the_bits_of_the_fp32_input():
    n = 0
    for r in device_run():
        if r["alpha_x3"] is None:
            continue
        n += 1
        assert np.array_equal(r["alpha"].view(np.uint32), r["alpha_x3"].view(np.uint32)), r["case"]
        assert r["rec"] == r["rec_x3"], r["case"]
    assert n == 252


@pytest.mark.parametrize("d,as_x3", [(128, False), (384, False), (1280, False), (1280, True)])
def test_stacked_equals_solo(d, as_x3):
    fx = cr.load_fixture(FIXTURE)
    w, b = fx["heads"][d]
    Ts = [2, 65, 1500, 13, 257, 901, 3, 400]
    kinds = ["noise", "boundary", "quiet_tail", "peaks"] * 2
    blocks = [cr.make_features(900 + i, T, d, kinds[i], 1.0, w) for i, T in enumerate(Ts)]
    stacked = diag_cif(blocks, w, b, as_x3=as_x3)
    for i, blk in enumerate(blocks):
        alpha, rec = diag_cif([blk], w, b, as_x3=as_x3)[0]
        assert np.array_equal(alpha.view(np.uint32), stacked[i][0].view(np.uint32)), (d, Ts[i])
        assert rec == stacked[i][1], (d, Ts[i])
    # a session with fewer than two frames among them gets no record and disturbs nobody
    short = diag_cif(blocks[:3], w, b, as_x3=as_x3, t_each=[2, 1, 1500])
    assert short[1][1]["seq"] == 0 and short[0][1] == stacked[0][1] and short[2][1] == stacked[2][1]


# ---- the switch, end to end ----------------------------------------------------------------------------------------
_models = {}


def own_model(tag):
    """Models of this file only: the head is set on them, which the shared models of the other test files must not see."""
    from whisperlivekit_amd.engine import HipWhisperModel
    if tag not in _models:
        _models[tag] = HipWhisperModel.synthetic("micro.en", 0)
    return _models[tag]


def make_proc(model, cif_device, teacher=None):
    from whisperlivekit_amd.backend import HipSimulStreamingASR, HipSimulStreamingOnlineProcessor
    g = H.golden_json("stream_micro_cif.json")
    asr = HipSimulStreamingASR("micro.en", hip_model=model, cif_device=cif_device, **H.asr_kwargs(g["cfg"]))
    proc = HipSimulStreamingOnlineProcessor(asr)
    proc.model.decision_log = []
    proc.model.teacher = dict(teacher) if teacher else None
    proc.fires = []
    fire0 = proc.model.fire_at_boundary

    def _fire(feature):
        r = fire0(feature)
        proc.fires.append(r)
        return r

    proc.model.fire_at_boundary = _fire
    return proc


def run_stream(proc, barrier=None):
    g = H.golden_json("stream_micro_cif.json")
    audio = H.stream_audio("micro_cif")
    words, t_end = [], 0.0
    for ev in g["events"]:
        assert ev["kind"] == "chunk"
        t_end += (ev["hi"] - ev["lo"]) / 16000
        proc.insert_audio_chunk(audio[ev["lo"]:ev["hi"]].copy(), t_end)
        if barrier is not None:
            barrier.wait()
        toks, _ = proc.process_iter()
        assert getattr(proc, "last_error", None) is None, proc.last_error
        words.append([(t.start, t.end, t.text) for t in toks])
    return words


def float64_decides_each_call(teacher):
    """Second pass, switch off, on a model without a head: the encoder output of every call is exported (here only) and
    the call's CIF case evaluated in float64 -> [decided] per call.  Its own decisions are the host path's."""
    proc = make_proc(own_model("host"), False, teacher)
    R = cr.load_fixture(FIXTURE)["R"]
    st = proc.model.state
    decided = []
    enc0 = proc.model._encode

    def _encode(segs):
        out = enc0(segs)
        d = proc.model.model.dims
        T = min(out[1], d.n_audio_ctx)
        x = proc.model.session.export("enc").reshape(d.n_audio_ctx, d.n_audio_state)[:T]
        decided.append(T >= 2 and cr.evaluate(x, st.cif_weight, st.cif_bias, R)["decided"])
        return out

    proc.model._encode = _encode
    try:
        run_stream(proc)
        return decided, [bool(f) for f in proc.fires]
    finally:
        proc.close()


def test_stream_with_the_switch_on_follows_the_golden_stream():
    from whisperlivekit_amd.align_att import DeviceFire
    g0 = H.golden_json("stream_micro_cif.json")
    golden_fire = [c["fire"] for c in g0["calls"]]
    state = {}

    def run(teacher):
        proc = make_proc(own_model("device"), True, teacher)
        try:
            words = run_stream(proc)
            assert all(isinstance(f, DeviceFire) for f in proc.fires)
            fires = [bool(f) for f in proc.fires]
            exports = dict(proc.model.session.export_calls)
            log = [list(x) for x in proc.model.decision_log]
        finally:
            proc.close()
        decided, host_fires = float64_decides_each_call(teacher)
        return dict(words=words, fires=fires, exports=exports, log=log, decided=decided, host_fires=host_fires)

    def compare(res):
        # calls are compared up to the first one whose CIF answer differs from the golden's - which float64 must not decide
        n = len(g0["calls"])
        k = next((i for i in range(min(n, len(res["fires"]))) if res["fires"][i] != golden_fire[i]), n)
        for i in range(min(k + 1, n)):
            if res["decided"][i]:
                assert res["fires"][i] == golden_fire[i], f"call {i}: float64 decides this case, the device disagrees"
        g = dict(g0, calls=g0["calls"][:min(k + 1, n)],
                 events=[ev for ev in g0["events"] if ev.get("call") is None or ev["call"] < k])
        emitted = res["words"][:sum(1 for ev in g["events"] if ev["kind"] == "chunk")]
        r = H.compare_decisions(g, res["log"][:len(g["calls"])], emitted)
        assert r["mismatch"] is None, r
        if r["tie_divergence"] is None:
            assert r["words_identical"], r
        state.update(compared=k, result=r)
        return r["tie_divergence"]

    res, ties = H.run_resynced(run, g0, compare)
    print("calls compared:", state["compared"], "of", len(g0["calls"]), "decided:", res["decided"], "ties:", ties)
    assert res["exports"].get("enc", 0) == 0, res["exports"]          # the encoder output never left the device
    assert res["host_fires"][:state["compared"]] == golden_fire[:state["compared"]]
    assert 4 * state["compared"] >= 3 * len(g0["calls"]), state
    assert sum(res["decided"]) >= 0.5 * len(res["decided"])


def test_eight_sessions_over_one_model_take_the_stacked_encode_lane():
    model = own_model("device")
    solo = make_proc(model, True)
    try:
        run_stream(solo)
        want = [bool(f) for f in solo.fires]
        want_log = [list(x) for x in solo.model.decision_log]
    finally:
        solo.close()
    before = model.engine_stats()
    procs = [make_proc(model, True) for _ in range(8)]
    barrier = threading.Barrier(8)
    errs = []

    def work(i):
        try:
            run_stream(procs[i], barrier)
        except Exception as e:       # noqa: BLE001 - reported below
            errs.append((i, repr(e)))
            barrier.abort()

    threads = [threading.Thread(target=work, args=(i,)) for i in range(8)]
    try:
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errs, errs
        after = model.engine_stats()
        batches = after["encode_batches"] - before["encode_batches"]
        sessions = after["encoded_sessions"] - before["encoded_sessions"]
        print(f"stacked encode lane: {sessions} session encodes in {batches} chains")
        assert batches > 0 and sessions > batches, (before, after)       # some chains held more than one session
        for p in procs:
            assert [bool(f) for f in p.fires] == want
            assert [list(x) for x in p.model.decision_log] == want_log
            assert p.model.session.export_calls.get("enc", 0) == 0
    finally:
        for p in procs:
            p.close()


def test_errors_and_removal():
    from whisperlivekit_amd import _lib
    from whisperlivekit_amd.engine import HipWhisperModel
    model = HipWhisperModel.synthetic("micro.en", 0)
    lib = model.lib
    try:
        d = model.dims.n_audio_state
        w = np.zeros(d, np.float32)
        s = model.new_session(batched=False)
        out = _lib.CifOut()
        assert lib.wlk_cif_result(s._h, C.byref(out)) == WLK_ERR_STATE            # no head
        s.append(H.stream_audio("micro_cif")[:16000])
        s.encode()
        assert lib.wlk_cif_result(s._h, C.byref(out)) == WLK_ERR_STATE            # encoded, still no head
        assert lib.wlk_model_set_cif(model._h, w.ctypes.data_as(C.c_void_p), d + 8, 0.0) == WLK_ERR_ARG
        with pytest.raises(_lib.WlkError):
            model.set_cif(np.zeros(d - 8, np.float32), 0.0)
        model.set_cif(w, -1.0)
        assert lib.wlk_cif_result(s._h, C.byref(out)) == WLK_ERR_STATE            # head, but nothing encoded with it
        s2 = model.new_session(beam=2, batched=False)                             # the record exists for any beam count
        assert lib.wlk_cif_result(s2._h, C.byref(out)) == WLK_ERR_STATE           # before any encode
        for sess in (s, s2):
            if sess is s2:
                sess.append(H.stream_audio("micro_cif")[:16000])
            sess.prof_begin()
            T = sess.encode()
            names = sess.prof_end(cap=128)
            assert names["cif_alpha"]["launches"] == 1 and names["cif_decide"]["launches"] == 1, sorted(names)
            rec = sess.cif_result()
            # w = 0, b = -1: every alpha is sigmoid(-1); n = round(T * 0.2689), nothing is resized
            assert rec.seq >= 1 and rec.resize_rounds == 0 and rec.n == int(np.rint(T / (1 + np.e)))
            assert abs(rec.total - T / (1 + np.e)) < 1e-3
        s.clear_audio()
        s.append(np.zeros(320, np.float32))                                       # one content frame
        assert s.encode() == 1
        assert lib.wlk_cif_result(s._h, C.byref(out)) == WLK_ERR_STATE            # an error, not a hang
        model.set_cif(None)
        s2.prof_begin()
        s2.encode()
        names = s2.prof_end(cap=128)
        assert "cif_alpha" not in names and "cif_decide" not in names and "enc_ln_post" in names
        assert lib.wlk_cif_result(s2._h, C.byref(out)) == WLK_ERR_STATE
        s.close()
        s2.close()
    finally:
        model.close()


def teardown_module(module):
    for m in _models.values():
        m.close()
    _models.clear()
    _RUN.clear()
