"""The line bench.py prints is what the driver parses out of a bounded stdout tail (round 5: a 21 KB line came back
`parsed: null`): it must stay small, carry the judged blocks, and never show a roofline fraction above 1."""
import copy
import importlib
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    sys.path.insert(0, ROOT)
    import bench as b
    return importlib.reload(b)


@pytest.fixture()
def round5_record():
    with open(os.path.join(ROOT, "profiles", "r05_bench_default.json")) as fh:
        return json.load(fh)


def _repriced(rec):
    """The round-5 record with its X3 families priced the round-6 way (bf16 flops issued / bf16 peak)."""
    rec = copy.deepcopy(rec)
    for roof in (rec["roofline"], rec["large_v3"]["roofline"]):
        roof["fp32_equiv_tflops"] = roof["achieved"]
        roof["achieved"] = round(6 * roof["achieved"], 2)
        roof["peak"] = 2500.0
        roof["frac"] = round(roof["achieved"] / 2500.0, 4)
        roof.pop("frac_at_rocprof_duration", None)
        for name, fam in roof["mfma_families"].items():
            if "x3" in name:
                fam.update(pipe="bf16", peak_tflops=2500.0, fp32_equiv_tflops=fam["achieved_tflops"],
                           achieved_tflops=round(6 * fam["achieved_tflops"], 2))
                fam["frac"] = round(fam["achieved_tflops"] / 2500.0, 4)
    return rec


def test_the_round5_pricing_is_refused(bench, round5_record):
    """profiles/r05_bench_default.json priced large-v3's X3 GEMM against the fp32 MFMA peak and printed 1.019: the line
    builder must refuse such a record instead of printing it."""
    assert round5_record["large_v3"]["roofline"]["frac"] > 1.0
    with pytest.raises(SystemExit, match="above 1"):
        bench.compact_line(round5_record, "bench_full.json")


def test_line_is_small_and_carries_the_judged_blocks(bench, round5_record):
    rec = _repriced(round5_record)
    line = bench.compact_line(rec, "bench_full.json")
    text = json.dumps(line, separators=(",", ":"))
    assert len(text) <= bench.LINE_CAP_BYTES <= 8000, len(text)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline", "eight_streams", "asr_plus_diarization_8_sessions", "large_v3",
                "parity_checked", "parity_ok", "full"):
        assert key in line, key
    roof = line["roofline"]
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(roof)
    assert roof["peak"] == 2500.0 and abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3 and roof["frac"] < 0.5
    assert "encode" in roof and "step" in roof and len(roof["families"]) >= 3
    cpu = line["cpu_baseline"]
    assert set(("value", "unit", "cores", "kind", "sample")) <= set(cpu) and len(cpu["sample"]) <= 150
    assert line["large_v3"]["roofline"]["frac"] <= 1.0 and line["large_v3"]["cpu_baseline"]["kind"] == "reference"
    assert "kernels" not in line and "launch_tags" not in line
    assert line["value"] == rec["value"] and line["parity_checked"]["decisions"] == rec["parity_checked"]["decisions"]


def test_oversized_optional_blocks_are_dropped_not_the_contract(bench, round5_record):
    rec = _repriced(round5_record)
    rec["pipeline"] = {"one_session": {"note": "x" * 700}, "eight_sessions": {"note": "y" * 9000}}
    line = bench.compact_line(rec, "bench_full.json")
    assert len(json.dumps(line, separators=(",", ":"))) <= bench.LINE_CAP_BYTES
    assert "roofline" in line and "cpu_baseline" in line and "parity_checked" in line


def test_fraction_check_walks_nested_blocks(bench):
    assert bench.check_fractions({"frac": 0.3, "encode": {"frac": 1.2}, "families": {"a": {"frac_of_hbm": 1.01}}}) == \
        ["roofline.encode.frac=1.2", "roofline.families.a.frac_of_hbm=1.01"]
    assert bench.check_fractions({"frac": 1.0, "x": [{"frac": 0.2}]}) == []


def test_sortformer_flops_formula(bench):
    """The diarizer's roofline numerator: one FastConformer block at d 512 / ff 2048 is ~14.3 MFLOP per frame plus the
    attention's T-dependent part (the round-5 review's own estimate: ~75 GFLOP per chunk at 291 frames)."""
    from whisperlivekit_amd.sortformer import SortformerDims
    d = SortformerDims()
    f = bench.sortformer_step_flops(d, 291, 200)
    assert 70e9 < f < 85e9, f
    # linear part scales with T, the attention part with T^2
    f1, f2 = bench.sortformer_step_flops(d, 100, 0), bench.sortformer_step_flops(d, 200, 0)
    assert 2.0 < f2 / f1 < 2.2


def test_dumped_outputs_are_float_arrays_a_caller_can_read_back(bench, tmp_path):
    """--dump-outputs: per session the committed words (call, start, end), their text and the decode decisions behind
    them, float arrays only, named by the session's audio seed."""
    class Model:
        decision_log = [[100, [(50257, 3), (1000, 7)]], [150, []], [200, [(2000, 9)]]]

    class Proc:
        model = Model()

    calls = [(0.1, 0.0, [], 0.5, []), (0.1, 0.0, [1.0], 1.0, [(0.2, 1.0, " hello")]),
             (0.1, 0.0, [1.4, 1.5], 1.5, [(1.0, 1.4, " wörld"), (1.4, 1.5, "!")])]
    bench.dump_outputs(str(tmp_path), [3], [Proc()], [calls])
    assert sorted(os.listdir(tmp_path)) == ["s3_decisions.npy", "s3_text.npy", "s3_words.npy"]
    import numpy as np
    words = np.load(tmp_path / "s3_words.npy")
    text = np.load(tmp_path / "s3_text.npy")
    dec = np.load(tmp_path / "s3_decisions.npy")
    assert words.dtype == np.float64 and text.dtype == np.float32 and dec.dtype == np.float64
    assert words.tolist() == [[1, 0.2, 1.0], [2, 1.0, 1.4], [2, 1.4, 1.5]]
    assert text.astype(np.uint8).tobytes().decode("utf-8").split("\0")[:-1] == [" hello", " wörld", "!"]
    assert dec.tolist() == [[0, 100, 50257, 3], [0, 100, 1000, 7], [1, 150, -1, -1], [2, 200, 2000, 9]]


def test_plain_run_options(bench, monkeypatch):
    """--full is off by default and --steps sets the number of timed steps (at least one)."""
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    args = bench.parse_args()
    assert (args.steps, args.warmup, args.full, args.dump_outputs) == (7, 2, False, "")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse_args()
