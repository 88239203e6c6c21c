"""CIF end-of-word head on the device, the parts that need no GPU: the ABI surface, the fixture
tests/golden/cif_device_kat.npz and its float64 helper (tests/cif_reference.py), and the fire_at_boundary hook over a
stub session."""
import os
import re

import numpy as np
import pytest

import cif_reference as cr
import helpers as H
from whisperlivekit_amd import _lib
from whisperlivekit_amd import policy as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(H.GOLDEN, "cif_device_kat.npz")
SYMBOLS = ("wlk_model_set_cif", "wlk_cif_result", "wlk_diag_cif")


def test_the_three_symbols_are_declared_listed_and_bound():
    header = open(os.path.join(ROOT, "include", "wlk_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in include/wlk_hip.h"
        assert name in _lib.EXPORTED_SYMBOLS, f"{name} is not in _lib.EXPORTED_SYMBOLS"

    class Recorder:          # _declare sets restype / argtypes on whatever getattr returns
        def __init__(self):
            self.seen = {}

        def __getattr__(self, name):
            fn = type("Fn", (), {})()
            self.seen[name] = fn
            return fn

    rec = Recorder()
    _lib._declare(rec)
    for name in SYMBOLS:
        assert name in rec.seen and rec.seen[name].argtypes is not None, f"{name} has no ctypes signature"
    # the record the kernel writes and the ctypes mirror have the same fields in the same order
    body = re.search(r"typedef struct wlk_cif_out \{(.*?)\} wlk_cif_out;", header, re.S).group(1)
    fields = re.findall(r"\b(?:int32_t|uint32_t|float)\s+(\w+);", body)
    assert fields == [f[0] for f in _lib.CifOut._fields_]
    assert fields[-1] == "seq"


def test_fixture_conditions():
    fx = cr.load_fixture(FIXTURE)
    assert fx["R"] >= 100 * fx["max_rel_dev"] > 0          # R is 100x the reference's own measured fp32 deviation
    want = [(d, T, k, s) for d in cr.D_VALUES for T in cr.T_VALUES for k in cr.KINDS for s in cr.SCALES]
    assert [(c["d"], c["T"], c["kind"], c["scale"]) for c in fx["cases"]] == want
    for d in cr.D_VALUES:
        assert np.array_equal(fx["heads"][d][0], cr.make_head(d)[0]) and fx["heads"][d][1] == -1.0
    per_d = {d: dict(n=0, undecided=0) for d in cr.D_VALUES}
    fires = holds = resized = 0
    for c, x, ev in cr.iter_fixture(FIXTURE):
        st = per_d[c["d"]]
        st["n"] += 1
        resized += ev["resize_rounds"] > 0
        if ev["resize_rounds"] == 0:
            assert ev["fire"] == cr.no_resize_cross_check(ev, c["T"]), c
        if not ev["decided"]:
            st["undecided"] += 1
            continue
        assert ev["fire"] == c["fire"], f"float64 disagrees with the reference on a decided case: {c}"
        fires += ev["fire"]
        holds += not ev["fire"]
    for d, st in per_d.items():
        assert 3 * st["undecided"] <= st["n"], (d, st)
    assert fires >= 8 and holds >= 8, (fires, holds)
    assert resized >= 20, resized


def test_float64_helper_against_the_existing_known_answers():
    import torch
    fx = cr.load_fixture(FIXTURE)
    ck = torch.load(os.path.join(H.GOLDEN, "cif_micro.pt"), map_location="cpu", weights_only=True)
    w, b = ck["weight"].float().numpy().reshape(-1), float(ck["bias"].reshape(-1)[0])
    kat = H.golden_json("cif_kat.json")
    decided = fires = 0
    for k in kat:
        ev = cr.evaluate(cr.kat_features(k), w, b, fx["R"])
        if ev["decided"]:
            decided += 1
            fires += ev["fire"]
            assert ev["fire"] == k["fire"], k
    assert decided >= 36 and fires >= 8, (decided, fires)     # at least three quarters decided, both answers present


def test_margin_rule_marks_a_quiet_tail_undecided():
    # sum(a) is an integer by construction; with a (near) zero last frame the integral over a[:-1] lands on it
    alpha = np.full(10, 0.5)
    alpha[-1] = 1e-9
    alpha[:-1] = (5.0 - 1e-9) / 9
    ev = cr.evaluate_alphas(alpha, 4e-5)
    assert not ev["decided"] and ev["why"] == "integ[T-2] vs cnt"
    alpha = np.full(10, 0.43)
    assert cr.evaluate_alphas(alpha, 4e-5)["decided"]
    with pytest.raises(IndexError):
        cr.evaluate(np.zeros((1, 8), np.float32), np.zeros(8, np.float32), 0.0, 4e-5)


# ---- the hook over a stub session ----------------------------------------------------------------------------------
class StubSession:
    def __init__(self, fire):
        self.fire, self.result_calls, self.export_calls_n = fire, 0, 0
        self.beam = 1

    def cif_result(self):
        self.result_calls += 1
        return _lib.CifOut(fire=int(self.fire))

    def export(self, what):
        self.export_calls_n += 1
        raise AssertionError("the device path must not export the encoder output")

    def close(self):
        pass


class StubModel:
    _wlk_hip_model = True

    def __init__(self, cif_device, fire=True):
        import types
        from whisperlivekit_amd.dims import ALIGNMENT_HEADS, MODEL_DIMS
        self.dims, self.alignment_heads, self.device = MODEL_DIMS["micro.en"], list(ALIGNMENT_HEADS["micro.en"]), 0
        self.decoder = types.SimpleNamespace(blocks=[None] * self.dims.n_text_layer)
        self.cif_device, self.heads_set, self.fire = cif_device, [], fire
        self.sessions = []

    is_multilingual = property(lambda self: self.dims.is_multilingual)
    num_languages = property(lambda self: self.dims.num_languages)

    def new_session(self, beam=1, max_audio_seconds=64.0):
        self.sessions.append(StubSession(self.fire))
        return self.sessions[-1]

    def ensure_cif(self, path, weight, bias):
        self.heads_set.append((path, np.asarray(weight).copy(), float(bias)))


class HostFeature:
    """What EncoderFeature is to the hook: a shape and, for the host path only, .numpy()"""

    def __init__(self, T, d=128, seed=0):
        self.shape, self.numpy_calls = (1, T, d), 0
        self._x = np.random.default_rng(seed).standard_normal((1, T, d)).astype(np.float32)

    def numpy(self):
        self.numpy_calls += 1
        return self._x


def make_hooks(cif_device, monkeypatch, fire=True, **cfg_over):
    from whisperlivekit_amd.align_att import HipAlignAttStandalone
    from whisperlivekit_amd.backend import build_config
    monkeypatch.delenv("WLK_CIF_DEVICE", raising=False)
    model = StubModel(cif_device, fire)
    cfg = build_config("micro.en", **cfg_over)
    return HipAlignAttStandalone(cfg=cfg, hip_model=model), model


CKPT = os.path.join(H.GOLDEN, "cif_micro.pt")


def test_switch_off_uses_the_host_function_only(monkeypatch):
    hooks, model = make_hooks(False, monkeypatch, cif_ckpt_path=CKPT)
    calls = []
    monkeypatch.setattr(P, "cif_fire_at_boundary", lambda f, w, b: calls.append(f.shape) or True)
    feat = HostFeature(25)
    assert hooks.fire_at_boundary(feat) is True
    assert calls == [(25, 128)] and feat.numpy_calls == 1
    assert model.heads_set == [] and model.sessions[0].result_calls == 0


@pytest.mark.parametrize("fire", [True, False])
def test_switch_on_reads_the_record_once_and_only_when_asked(monkeypatch, fire):
    hooks, model = make_hooks(True, monkeypatch, fire=fire, cif_ckpt_path=CKPT)
    assert len(model.heads_set) == 1 and model.heads_set[0][0] == CKPT and model.heads_set[0][1].shape == (128,)
    monkeypatch.setattr(P, "cif_fire_at_boundary", lambda *a: pytest.fail("host path taken with the switch on"))
    feat = HostFeature(25)
    got = hooks.fire_at_boundary(feat)
    sess = model.sessions[0]
    assert sess.result_calls == 0 and feat.numpy_calls == 0          # nothing is read at the hook
    taken = "yes" if (got or False) else "no"                        # `fire_detected or is_last`, as the policy does
    assert taken == ("yes" if fire else "no")
    assert bool(got) is fire and bool(got) is fire
    assert sess.result_calls == 1 and feat.numpy_calls == 0


def test_environment_switch(monkeypatch):
    from whisperlivekit_amd.align_att import HipAlignAttStandalone
    from whisperlivekit_amd.backend import build_config
    monkeypatch.setenv("WLK_CIF_DEVICE", "1")
    model = StubModel(False)
    HipAlignAttStandalone(cfg=build_config("micro.en", cif_ckpt_path=CKPT), hip_model=model)
    assert len(model.heads_set) == 1


@pytest.mark.parametrize("T", [0, 1])
def test_too_few_frames_raise_at_the_hook(monkeypatch, T):
    hooks, model = make_hooks(True, monkeypatch, cif_ckpt_path=CKPT)
    with pytest.raises(IndexError):
        hooks.fire_at_boundary(HostFeature(T))
    assert model.sessions[0].result_calls == 0


@pytest.mark.parametrize("over,want", [(dict(), True), (dict(never_fire=True), False),
                                       (dict(cif_ckpt_path=CKPT, never_fire=True), False)])
def test_always_and_never_fire_do_not_touch_the_device(monkeypatch, over, want):
    hooks, model = make_hooks(True, monkeypatch, **over)
    feat = HostFeature(25)
    assert hooks.fire_at_boundary(feat) is want
    assert model.sessions[0].result_calls == 0 and feat.numpy_calls == 0


def test_one_head_per_shared_model(tmp_path):
    """engine.HipWhisperModel.ensure_cif without a GPU: the first path wins, another one is refused."""
    import threading
    from whisperlivekit_amd.engine import HipWhisperModel
    m = HipWhisperModel.__new__(HipWhisperModel)
    m._cif_lock, m._cif_path, sets = threading.Lock(), None, []
    m.set_cif = lambda w, b: sets.append((w, b))
    m.ensure_cif("a.pt", np.zeros(4, np.float32), -1.0)
    m.ensure_cif("a.pt", np.zeros(4, np.float32), -1.0)
    assert len(sets) == 1
    with pytest.raises(ValueError):
        m.ensure_cif("b.pt", np.zeros(4, np.float32), -1.0)
    m._h = None                                   # nothing to destroy
