#!/usr/bin/env python
"""Every Whisper entry point that enqueues decoder layers, once, on synthetic tiny.en (seed 0; GPU only) - what a change to
the composition of the decoder chain (csrc/decoder_chain.h) is compared on, tree against tree:

    python scripts/decoder_chain_probe.py [--out DIR]          run; with --out every result below is stored as DIR/<name>.npy
    rocprofv3 --kernel-trace --stats --output-format csv -d D -o t -- python scripts/decoder_chain_probe.py --no-batched-engine
                                                            the same run under the profiler (no other tracing, one run per tree)
    python scripts/decoder_chain_probe.py --compare-out A B [C]  largest |A - B| per array; with C also |A - C| (A, C: two runs
                                                            of one tree, B: the other tree)
    python scripts/decoder_chain_probe.py --compare-trace A.csv B.csv   two *_kernel_trace.csv: calls per kernel name side by
                                                            side, and whether the names come in the same order

Beam-1 session: prefill of 12 tokens (merged last+sot read-out) and of 3 (<= 8 rows, n_tok > 1), two decode(first=0) + select
(the graph step), a short decode_until_stop (the step + read-out replay).  Beam-3 session: prefill of 3 x 12 rows, kv_reorder +
decode, two decode_ancestry.  Debug session: prefill and a step (plain cross-attention, cross_qk).  Profiling session: prefill
and an eager step, the tags and launch counts of prof_end.  find_alignment (raw scores) and a head survey of 5 tokens.  Stacked
prefill of prompts of 12 / 20 / 33 tokens.  Window group: step of 1 row and of 3, a run_pick burst, a draft verify, a group
find_alignment.  Batch engine: a loop of one attached session (single-row steps) and - unless --no-batched-engine: how many
rows share a step depends on when the threads arrive, so that leg's launches differ from run to run of ONE tree - two
attached sessions looping side by side.  Stored: logits_last / logits_sot / dec_x / attn_last / the alignment window after
every call, every top-k pair and frame, cross_qk, the loops' tokens, frames and log-probability sums, and what the group,
the alignment and the survey calls hand back.
"""
import csv
import ctypes as C
import glob
import os
import sys
import threading

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SOT, NOTS, EOT, TS0 = 50257, 50362, 50256, 50363


def run(out_dir, batched_engine=True):
    from whisperlivekit_amd import _lib, synth
    from whisperlivekit_amd.engine import HipWhisperModel, HipWindowGroup
    if _lib.device_count() < 1:
        raise SystemExit("decoder_chain_probe: no HIP device (there is nothing to run without one)")
    kept = {}

    def keep(name, *arrays):
        for i, a in enumerate(arrays):
            kept[f"{name}.{i}"] = np.array(a, copy=True)

    model = HipWhisperModel.synthetic("tiny.en", 0)
    dims, lib = model.dims, model.lib
    rng = np.random.default_rng(3)
    opened = []

    def prompt(n):
        return np.concatenate([[SOT, NOTS], rng.integers(300, 40000, size=n - 2)]).astype(np.int64)

    def session(beam=1, seed=0, batched=False):
        s = model.new_session(beam=beam, batched=batched)
        s.append(synth.speech_like(3.0 + seed, seed=40 + seed))
        opened.append(s)
        return s, s.encode()

    def snap(name, s, cml, sot=False, window=True):
        """the exports of the last decode and its read-out"""
        keep(name + ".logits", s.export("logits_last", s.beam * dims.n_vocab))
        if sot:
            keep(name + ".sot", s.export("logits_sot", s.beam * dims.n_vocab))
        keep(name + ".dec_x", s.export("dec_x"))
        keep(name + ".select", *s.select([], [], [], 2, cml), s.export("attn_last"))
        if window:
            keep(name + ".window", s.export("xattn_w:0"))

    def loop_params(cml, budget):
        return _lib.LoopParams(sot_index=0, is_last=0, frame_threshold=-10 ** 6, rewind_threshold=10 ** 6, last_attend_frame=0,
                               max_text_len=dims.n_text_ctx, budget=budget, eot=EOT, dec_pad=SOT, no_speech_token=-1,
                               no_speech_threshold=1.0, content_mel_len=cml)

    def keep_loop(name, out):
        keep(name, out.new_tokens, out.step_tokens, out.step_frames, out.step_sum_logprobs,
             [out.stop_reason, out.last_attend_frame, out.decode_calls], [out.no_speech_prob, out.sum_logprob])

    # ---- beam 1
    s, cml = session()
    s.decode(prompt(12)[None], first=True, sot_index=0)
    snap("b1.prefill12", s, cml, sot=True)
    s.decode(prompt(3)[None], first=True, sot_index=0)
    snap("b1.prefill3", s, cml, sot=True)
    for i, t in enumerate((1234, 2345)):
        s.decode(np.asarray([[t]]), first=False)
        snap(f"b1.step{i}", s, cml)
    keep_loop("b1.loop", s.decode_until_stop(prompt(12), loop_params(cml, 4), [EOT], []))
    keep("b1.loop.logits", s.export("logits_last", dims.n_vocab), s.export("dec_x"))

    # ---- beam 3
    s3, cml3 = session(beam=3, seed=1)
    s3.decode(np.tile(prompt(12), (3, 1)), first=True, sot_index=0)
    snap("b3.prefill", s3, cml3, sot=True)
    s3.kv_reorder([1, 0, 0])
    s3.decode(np.asarray([[700], [800], [900]]), first=False)
    snap("b3.step", s3, cml3)
    for i, (toks, src) in enumerate((([701, 801, 901], [0, 0, 2]), ([702, 802, 902], [2, 1, 1]))):
        s3.decode_ancestry(toks, src)
        snap(f"b3.anc{i}", s3, cml3)

    # ---- debug: the plain cross-attention kernel and its raw scores
    sd, cmld = session(seed=2)
    sd.set_debug(True)
    sd.decode(prompt(12)[None], first=True, sot_index=0)
    snap("dbg.prefill", sd, cmld, sot=True)
    keep("dbg.prefill.qk", *[sd.export(f"cross_qk:{l}") for l in range(dims.n_text_layer)])
    sd.decode(np.asarray([[1234]]), first=False)
    snap("dbg.step", sd, cmld)
    keep("dbg.step.qk", *[sd.export(f"cross_qk:{l}") for l in range(dims.n_text_layer)])

    # ---- profiling: eager launches, the tags bench.py's roofline reads
    sp, cmlp = session(seed=3)
    sp.prof_begin()
    sp.decode(prompt(12)[None], first=True, sot_index=0)
    sp.decode(np.asarray([[1234]]), first=False)
    prof = sp.prof_end(cap=128)
    keep("prof", np.asarray(sorted(prof)), [prof[k]["launches"] for k in sorted(prof)])
    snap("prof.step", sp, cmlp)

    # ---- find_alignment's raw-score pass and a head survey (flash whatever the row count, kept queries)
    sa, cmla = session(seed=4)
    words = np.concatenate([[SOT, NOTS], rng.integers(300, 40000, size=6), [EOT]]).astype(np.int64)
    keep("align", *sa.find_alignment(words, 1, EOT, 2 * cmla, want_cost=True))
    keep("survey", *sa.head_survey(prompt(5), 2 * cmla))

    # ---- stacked prefill of three sessions: 12, 20 and 33 tokens (the last one crosses a 32-row tile)
    stack = [session(seed=5 + i) for i in range(3)]
    prompts = [prompt(n) for n in (12, 20, 33)]
    handles = (C.c_void_p * 3)(*[x[0]._h for x in stack])
    flat = np.ascontiguousarray(np.concatenate(prompts))
    n_tok, sot, taken = np.asarray([12, 20, 33], np.int32), np.zeros(3, np.int32), np.zeros(3, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    _lib.check(lib.wlk_diag_prefill_stack(handles, vp(flat), vp(n_tok), vp(sot), 3, vp(taken)))
    if taken.tolist() != [1, 1, 1]:
        raise SystemExit(f"decoder_chain_probe: the stack took {taken.tolist()}")
    for i, (x, c) in enumerate(stack):
        snap(f"stack{i}", x, c, sot=True)

    # ---- window group: steps of 1 and 3 rows, a burst, a draft verify, a group alignment
    group = HipWindowGroup(model, 8)
    state = dict(first_step=False, without_timestamps=True, timestamp_begin=TS0, eot=EOT, no_timestamps=NOTS, ts_mode=0,
                 ts_bound=TS0, max_initial=-1)
    wins = [x[0] for x in stack]
    for x, p in zip(wins, prompts):
        x.set_rules([SOT, NOTS], [220, EOT])
    keep("group.step1", *group.step_pick(wins[:1], [1500], [state]), group.export_logits(0))
    keep("group.step3", *group.step_pick(wins, [1600, 1601, 1602], [state] * 3), *[group.export_logits(r) for r in range(3)])
    burst = group.run_pick(wins, [1700, 1701, 1702], [state] * 3, [4, 4, 4], 4)
    keep("group.burst", *[a for row in burst for a in row], *[group.export_logits(r) for r in range(3)])
    gwords = np.concatenate([[SOT, NOTS], rng.integers(300, 40000, size=12), [EOT]]).astype(np.int64)
    if not group.verify_fits(12, 5) or not all(group.fits(len(gwords), 2 * c) for _, c in stack[:2]):
        raise SystemExit("decoder_chain_probe: the group refuses the probe's verify or alignment shape")
    first = dict(state, first_step=True)
    got = group.verify([(x, list(prompt(12)), [int(t) for t in rng.integers(300, 40000, size=5)], 0, first, None)
                        for x in wins[:2]], want_picks=True)
    keep("group.verify", *[a for r in got for a in ([r["accepted"], r["next_token"]], [r["next_logprob"], r["sum_logprob"],
                                                                                         r["no_speech_prob"]], *r["picks"])])
    for i, x in enumerate(wins[:2]):
        keep(f"group.verify.logits{i}", x.export("logits_last", dims.n_vocab))
    got = group.find_alignment([(x, gwords, 1, EOT, 2 * c) for x, c in stack[:2]], want_cost=True, want_trace=True)
    keep("group.align", *[a for r in got for a in r])
    group.close()

    # ---- the batch engine: single-row steps (the one-row query fold), then two loops side by side
    se, cmle = session(seed=8, batched=True)
    keep_loop("engine.one", se.decode_until_stop(prompt(12), loop_params(cmle, 4), [EOT], []))
    if batched_engine:
        pair = [session(seed=9 + i, batched=True) for i in range(2)]
        pair_prompts = [prompt(12), prompt(14)]
        gate, outs = threading.Barrier(2), [None, None]

        def loop(i):
            gate.wait()
            outs[i] = pair[i][0].decode_until_stop(pair_prompts[i], loop_params(pair[i][1], 8), [EOT], [])
        threads = [threading.Thread(target=loop, args=(i,)) for i in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        for i in range(2):
            keep_loop(f"engine.pair{i}", outs[i])
        st = model.engine_stats()
        print(f"decoder_chain_probe: engine iterations {st['iterations']}, batched steps {st['batched_steps']}, "
              f"rows in them {st['batched_rows']}")
        if st["batched_steps"] < 1:
            raise SystemExit("decoder_chain_probe: the two loops never shared an engine step - the batched step was not reached")
    for x in opened:
        x.close()
    model.close()
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        for name, a in kept.items():
            np.save(os.path.join(out_dir, name + ".npy"), a)
    print(f"decoder_chain_probe: {len(kept)} arrays" + (f" stored under {out_dir}" if out_dir else ""))


def load(d):
    return {os.path.basename(p)[:-4]: np.load(p) for p in sorted(glob.glob(os.path.join(d, "*.npy")))}


def largest(a, b):
    if a.shape != b.shape:
        return float("inf")
    if a.dtype.kind in "US":
        return 0.0 if np.array_equal(a, b) else float("inf")
    if not a.size:
        return 0.0
    x, y = a.astype(np.float64), b.astype(np.float64)
    same = (x == y) | (np.isnan(x) & np.isnan(y))         # equal infinities are no difference
    return float(np.abs(np.where(same, 0.0, x - y)).max())


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def compare_out(a_dir, b_dir, c_dir=None):
    a, b = load(a_dir), load(b_dir)
    c = load(c_dir) if c_dir else None
    if set(a) != set(b) or (c is not None and set(a) != set(c)):
        raise SystemExit("decoder_chain_probe: the runs did not store the same arrays")
    worst_b = worst_c = 0.0
    bad = []
    for name in sorted(a):
        db = 0.0 if same_bits(a[name], b[name]) else max(largest(a[name], b[name]), np.finfo(np.float64).tiny)
        dc = 0.0
        if c is not None and not same_bits(a[name], c[name]):
            dc = max(largest(a[name], c[name]), np.finfo(np.float64).tiny)
            print(f"not reproducible on one tree: {name}, largest difference {dc:g}")
        if db > dc:
            bad.append(name)
            print(f"differs between the trees: {name}, largest difference {db:g} (one tree against itself: {dc:g})")
        worst_b, worst_c = max(worst_b, db), max(worst_c, dc)
    print(f"{len(a)} arrays, {sum(v.size for v in a.values())} values")
    if c is not None:
        print(f"{a_dir} against {c_dir}: bit-identical {worst_c == 0.0}, largest difference {worst_c:g}")
    print(f"{a_dir} against {b_dir}: bit-identical {worst_b == 0.0}, largest difference {worst_b:g}")
    return 1 if bad else 0


def kernel_names(path):
    with open(path, newline="") as fh:
        rows = list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return [r["Kernel_Name"] for r in rows]


def compare_trace(a_csv, b_csv):
    a, b = kernel_names(a_csv), kernel_names(b_csv)
    count = lambda names: {n: names.count(n) for n in dict.fromkeys(names)}
    ca, cb = count(a), count(b)
    print(f"{'kernel':<72}{'parent':>8}{'new':>8}")
    for n in sorted(set(ca) | set(cb), key=lambda n: (-ca.get(n, 0), n)):
        print(f"{n[:70]:<72}{ca.get(n, 0):>8}{cb.get(n, 0):>8}")
    print(f"{'all kernels':<72}{len(a):>8}{len(b):>8}")
    print(f"# per-name counts equal: {ca == cb}; the two traces are the same kernel names in the same order: {a == b}")
    return 0 if a == b else 1


if __name__ == "__main__":
    if "--compare-out" in sys.argv:
        sys.exit(compare_out(*sys.argv[sys.argv.index("--compare-out") + 1:][:3]))
    if "--compare-trace" in sys.argv:
        i = sys.argv.index("--compare-trace")
        sys.exit(compare_trace(sys.argv[i + 1], sys.argv[i + 2]))
    run(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None, "--no-batched-engine" not in sys.argv)
