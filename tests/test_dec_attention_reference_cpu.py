"""The references of tests/dec_attention_reference.py against independent statements, on every case of
tests/dec_attention_cases.py, without a GPU: the float64 form against an explicit torch float64 computation, the ancestry
model against a simulation that keeps every hypothesis's history as a list, and the float32 restatement against the
tolerance it defines (a case whose restatement is not finite could not be judged)."""
import numpy as np
import pytest
import torch

import dec_attention_cases as DC
import dec_attention_reference as DR


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).double()


def self_reference_args(case, route):
    """-> keyword arguments of DR.self_attention for `route` on `case` (identity rows / table for a plain case)"""
    kw = dict(row_cache=None, anc=None)
    if case["form"] == "rows":
        kw["row_cache"] = case["row_cache"]
    elif case["form"] == "anc":
        kw["anc"] = case["anc"]
    return kw


def torch_self(case):
    c = case
    qkv, kc, vc = t64(c["qkv"]), t64(c["kc"]), t64(c["vc"])
    d, H, n_tok, n_rows = c["d"], c["H"], c["n_tok"], c["n_rows"]
    out = torch.zeros(qkv.shape[0], d, dtype=torch.float64)
    for r in range(qkv.shape[0]):
        b, p = divmod(r, n_tok)
        off = int(c["offsets"][b] if len(c["offsets"]) > 1 else c["offsets"][0])
        n = off + p + 1
        pos = torch.arange(n)
        if c["form"] == "anc":
            src = torch.from_numpy(c["anc"][b, :n].astype(np.int64)).clamp(max=n_rows - 1)
        else:
            src = torch.full((n,), int(c["row_cache"][b]) if c["form"] == "rows" else b)
        K = kc[src, pos].view(n, H, 64).transpose(0, 1)
        V = vc[src, pos].view(n, H, 64).transpose(0, 1)
        w = torch.softmax(torch.einsum("hd,hnd->hn", qkv[r, :d].view(H, 64), K), dim=-1)
        out[r] = torch.einsum("hn,hnd->hd", w, V).reshape(d)
    return out.numpy()


def torch_cross(case, route):
    c = case
    d, H, R, T = c["d"], c["H"], c["R"], c["T"]
    if route == "C2":
        h = torch.nn.functional.layer_norm(t64(c["x"]), (d,), t64(c["gamma"]), t64(c["beta"]), 1e-5)
        q = torch.nn.functional.linear(h, t64(c["wq"]), None if c["bq"] is None else t64(c["bq"])) * float(np.float32(c["scale"]))
    else:
        q = t64(c["q"])
    sets = torch.from_numpy(c["row_kv"].astype(np.int64)) if route == "C4" else torch.zeros(R, dtype=torch.int64)
    K = t64(c["k"])[sets].view(R, T, H, 64)
    V = t64(c["v"])[sets].view(R, T, H, 64)
    s = torch.einsum("rhd,rthd->rht", q.view(R, H, 64), K)
    w = torch.softmax(s, dim=-1)
    out = torch.einsum("rht,rthd->rhd", w, V).reshape(R, d)
    if route == "C3":
        out = (torch.nn.functional.linear(out, t64(c["wo"]), t64(c["bo"])) + t64(c["resid"]))[:1]
    return out.numpy(), w.numpy(), s.numpy()


@pytest.mark.parametrize("name", DC.SELF_NAMES)
def test_self_attention_reference(name):
    case = DC.build(name)
    kw = self_reference_args(case, None)
    ref = DR.self_attention(case["qkv"], case["kc"], case["vc"], case["n_tok"], case["offsets"], case["H"], np.float64, **kw)
    assert np.abs(ref - torch_self(case)).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    f32 = DR.self_attention(case["qkv"], case["kc"], case["vc"], case["n_tok"], case["offsets"], case["H"], np.float32, **kw)
    entry, fail = DR.judge("out", f32, ref, f32)
    assert fail is None and np.isfinite(entry["restatement_err"]), (entry, fail)
    if case["anc_alt"] is not None:      # the alternative table is the same operation
        alt = DR.self_attention(case["qkv"], case["kc"], case["vc"], 1, case["offsets"], case["H"], np.float64, anc=case["anc_alt"])
        assert np.array_equal(alt, ref)
    # nothing at or behind a key count is read
    poisoned = DC.stale(case, np.nan)
    again = DR.self_attention(case["qkv"], poisoned["kc"], poisoned["vc"], case["n_tok"], case["offsets"], case["H"], np.float64, **kw)
    assert np.array_equal(again, ref)


@pytest.mark.parametrize("name", DC.CROSS_NAMES)
def test_cross_attention_reference(name):
    case = DC.build(name)
    routes = sorted(set(case["routes"]) | set(case["refused"]))
    assert routes
    for route in routes:
        if route in ("C2", "C3") and ("x" if route == "C2" else "wo") not in case:
            continue
        if route == "C3" and case["R"] != 1:
            continue
        ref = DR.cross_reference(case, route, np.float64)
        f32 = DR.cross_reference(case, route, np.float32)
        out, w, s = torch_cross(case, route)
        scale = max(1.0, np.abs(ref["out"]).max())
        assert np.abs(ref["out"] - out).max() <= 1e-11 * scale, route
        assert np.abs(ref["scores"] - s).max() <= 1e-11 * max(1.0, np.abs(s).max()), route
        for (rank, beam, ring_row), row in ref["align"].items():
            r = [i for i in range(case["R"]) if case["beam_of_row"][i] == beam and case["ring_row"][i] == ring_row]
            h = int(np.flatnonzero(case["head_rank"] == rank)[0])
            assert len(r) == 1 and np.abs(row - w[r[0], h]).max() <= 1e-12, route
            assert abs(row.sum() - 1.0) <= 1e-12
        assert len(ref["align"]) == (0 if case["head_rank"] is None else case["R"] * int((case["head_rank"] >= 0).sum()))
        for key in ("out", "scores"):
            entry, fail = DR.judge(key, f32[key], ref[key], f32[key])
            assert fail is None and np.isfinite(entry["restatement_err"]), (route, key, entry, fail)
        for slot, row in ref["align"].items():
            entry, fail = DR.judge("align", f32["align"][slot], row, f32["align"][slot])
            assert fail is None, (route, slot, entry, fail)


def test_no_case_is_left_out():
    for name in DC.SELF_NAMES + DC.CROSS_NAMES:
        case = DC.build(name)
        assert DC.expected_routes(case) or case["refused"], name
    assert {f"keys_{n}" for n in DC.KEY_COUNTS} <= set(DC.SELF_NAMES)


def simulate_histories(seq, n_rows, ctx_len):
    """every hypothesis's history as a list of the physical rows that hold its positions"""
    hist = None
    for ctl, offset in seq:
        if ctl[7]:
            hist = [[b] * offset for b in range(n_rows)]
        # a position the source never wrote itself lies in the source's own row
        padded = [h + [b] * max(0, offset - len(h)) for b, h in enumerate(hist)]
        hist = [padded[int(ctl[b])][:offset] + [b] for b in range(n_rows)]
    return hist


@pytest.mark.parametrize("name", sorted(DC.ANC_SEQUENCES))
def test_ancestry_model_against_history_lists(name):
    spec = DC.ANC_SEQUENCES[name]
    seq = DC.anc_sequence(name, **spec)
    n_rows, ctx_len = spec["n_rows"], spec["ctx_len"]
    table = np.full((n_rows + 1, ctx_len), 0xA5, np.uint8)       # stale content and a guard row
    for u, (ctl, offset) in enumerate(seq):
        table = DR.anc_update(table, ctl, offset, n_rows)
        hist = simulate_histories(seq[:u + 1], n_rows, ctx_len)
        for b in range(n_rows):
            want = (hist[b] + [b] * ctx_len)[:ctx_len]
            assert table[b].tolist() == want, (u, b)
        assert np.all(table[n_rows] == 0xA5)


def test_copy_models():
    rng = np.random.default_rng(3)
    src = rng.standard_normal((2, 3, 8, 4)).astype(np.float32)
    g = DR.kv_gather(src, [2, 0, 2], 5)
    assert g.shape == (2, 3, 5, 4) and np.array_equal(g[1, 0], src[1, 2, :5]) and np.array_equal(g[0, 1], src[0, 0, :5])
    qkv = rng.standard_normal((6, 12)).astype(np.float32)
    kc, vc = DR.kv_append(np.zeros((3, 8, 4), np.float32), np.zeros((3, 8, 4), np.float32), qkv, 2, [3])
    assert np.array_equal(kc[1, 4], qkv[3, 4:8]) and np.array_equal(vc[2, 3], qkv[4, 8:]) and not kc[:, :3].any() and not kc[:, 5:].any()
    kc, vc = DR.kv_append(np.zeros((3, 8, 4), np.float32), np.zeros((3, 8, 4), np.float32), qkv[:3], 1, [7, 0, 2], [2, 0, 1])
    assert np.array_equal(kc[2, 7], qkv[0, 4:8]) and np.array_equal(vc[0, 0], qkv[1, 8:]) and np.array_equal(kc[1, 2], qkv[2, 4:8])
