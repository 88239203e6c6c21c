"""Device-resident Sortformer sessions, the parts that need no GPU: the C ABI's cache-parameter struct against
SpkCacheParams, the new entry points declared / exported, the device_state switch, and no host fallback."""
import ctypes as C
import dataclasses
import os
import re

import pytest

from whisperlivekit_amd import _lib
from whisperlivekit_amd import sortformer as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SESSION_SYMBOLS = ("wlk_sf_session_create", "wlk_sf_session_destroy", "wlk_sf_session_step_pcm", "wlk_sf_session_step",
                   "wlk_sf_session_update", "wlk_sf_session_get_state", "wlk_sf_session_set_state")


def header_struct_fields(name):
    text = open(os.path.join(ROOT, "include", "wlk_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        fields += [(n.strip().lstrip("*"), ctype) for n in names.split(",")]
    return fields


def test_cache_params_struct_mirrors_spkcache_params_field_by_field():
    py = [(f.name, f.type) for f in dataclasses.fields(sf.SpkCacheParams)]
    ct = [(n, t) for n, t in _lib.SfCacheParams._fields_]
    assert [n for n, _ in ct] == [n for n, _ in py]
    for (n, t), (_, pt) in zip(ct, py):
        assert (t is C.c_int32) == (pt in (int, "int")) and (t is C.c_float) == (pt in (float, "float")), n
    hdr = header_struct_fields("wlk_sf_cache_params")
    assert [n for n, _ in hdr] == [n for n, _ in ct]
    assert all((t == "float") == (ct_t is C.c_float) for (_, t), (_, ct_t) in zip(hdr, ct))
    # values survive the trip into the struct (the fp32 fields round like np.float32)
    cp = sf.cache_params_struct(sf.SpkCacheParams())
    assert (cp.spkcache_len, cp.fifo_len, cp.spkcache_update_period, cp.max_index) == (188, 188, 144, 99999)
    assert cp.sil_threshold == float(__import__("numpy").float32(0.2))


def test_state_struct_matches_the_header():
    hdr = header_struct_fields("wlk_sf_state")
    assert [n for n, _ in hdr] == [n for n, _ in _lib.SfState._fields_]


def test_session_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "wlk_hip.h")).read()
    lib = _lib.load()
    for name in SESSION_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert getattr(lib, name).argtypes, name


@pytest.mark.parametrize("arg,env,want", [(None, None, False), (None, "1", True), (None, "0", False), (None, "on", True),
                                          (True, "0", True), (False, "1", False), (None, "", False)])
def test_device_state_resolution(monkeypatch, arg, env, want):
    if env is None:
        monkeypatch.delenv("WLK_SF_DEVICE_STATE", raising=False)
    else:
        monkeypatch.setenv("WLK_SF_DEVICE_STATE", env)
    assert sf.resolve_device_state(arg) is want


def test_new_device_state_without_a_model_on_a_gpu_raises():
    """No host fallback: a model handle that is not a live GPU model (what a machine without a GPU leaves) is an error
    of the library, not a quiet host state."""
    m = object.__new__(sf.HipSortformerModel)
    m.lib, m._h, m.cache, m._mel = _lib.load(), C.c_void_p(), sf.SpkCacheParams(), None
    import weakref
    m._states = weakref.WeakSet()
    with pytest.raises(_lib.WlkError):
        m.new_device_state()
    if _lib.device_count() == 0:
        with pytest.raises(_lib.WlkError):
            sf.HipSortformerModel.synthetic(sf.SortformerDims(fc_layers=0, tf_layers=0), device_state=True)
