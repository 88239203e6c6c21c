"""Plain numpy statements of NLLB's ragged decoder cross-attention (csrc/nllb_batch.hip:
nllb_cross_attention_ragged_kernel<false|true>), float64 and float32 by one function with the number type as an argument.

Row r of q [n_rows][d] attends, head by head (64 features each), to the first lengths[r] key rows of its own block:
score_j = q_h . k_jh (the scale is folded into q), softmax over the keys, out_h = sum_j p_j v_jh.  The align form also keeps
p of every head h with head_rank[h] >= 0 at probs[head_rank[h]][r][0 .. lengths[r]).

`mistake` switches one deliberate error on (MISTAKES); test_cross_ragged_reference_cpu.py requires that some named case
tells every one of them from the reference at the GPU test's tolerance (select_reference.value_tolerance: 4 x the float32
restatement's error on the case, floor 2^-22 max(1, |reference|)).  No torch in here.

OUTPUT_FACTOR: families whose kernel-to-restatement factor is not the default 4, with the case that measured it (none)."""
import numpy as np

from select_reference import abs_err, value_tolerance

OUTPUT_FACTOR = {}
HEAD = 64
MAX_ROWS = 8            # kNlBatchMaxRows: rows per rank of the alignment block
MISTAKES = ("neighbours_length", "one_key_too_many", "probs_not_normalised", "rank_table_ignored")


def attention(case, dt=np.float64, mistake=None):
    """-> dict(out [n_rows][d], probs [n_rank][8][stride] with NaN where nothing is stored - or None without head_rank,
    sums [n_rows][H]: the sum of every (row, head)'s weights)"""
    c = case
    R, H, d = c["n_rows"], c["H"], c["d"]
    lengths = np.asarray(c["lengths"])
    if mistake == "neighbours_length":
        lengths = np.roll(lengths, 1)
    rank = c["head_rank"]
    if rank is not None and mistake == "rank_table_ignored":
        rank = np.arange(H) % c["n_rank"]
    out = np.empty((R, d), dt)
    sums = np.empty((R, H), dt)
    probs = None if rank is None else np.full((c["n_rank"], MAX_ROWS, c["stride"]), np.nan, dt)
    for r in range(R):
        T = min(int(lengths[r]) + (1 if mistake == "one_key_too_many" else 0), c["kv_rows"][r])
        block = c["blocks"][r][:T, c["kv_off"]:c["kv_off"] + 2 * d].astype(dt)
        for h in range(H):
            sl = slice(h * HEAD, (h + 1) * HEAD)
            q = c["q"][r, sl].astype(dt)
            k, v = block[:, sl], block[:, d:][:, sl]
            s = (k * q[None, :]).sum(axis=1, dtype=dt)
            with np.errstate(invalid="ignore"):
                e = np.exp(s - s.max(), dtype=dt)
                p = e / e.sum(dtype=dt)
            out[r, sl] = (p[:, None] * v).sum(axis=0, dtype=dt)
            sums[r, h] = p.sum(dtype=dt)
            if rank is not None and rank[h] >= 0:
                n = min(T, c["stride"])
                probs[rank[h], r, :n] = (e if mistake == "probs_not_normalised" else p)[:n]
    return dict(out=out, probs=probs, sums=sums)


def compare(ref, f32, got, keys=("out", "probs", "sums")):
    """as word_align_reference.compare; a NaN in the reference's probs marks a word nothing may be stored to"""
    report, failures = {}, []
    for key in keys:
        if got.get(key) is None or ref.get(key) is None:
            continue
        allowed, e32 = value_tolerance(ref[key], f32[key])
        err = abs_err(got[key], ref[key])
        worst = int(np.argmax(err - allowed))
        report[key] = dict(restatement_err=e32, kernel_err=float(err.max()), allowed=float(allowed.reshape(-1)[worst]),
                           ratio=float(err.max() / e32) if e32 > 0 else None)
        if (err > allowed).any():
            failures.append(f"{key}: error {err.reshape(-1)[worst]:.3e} > allowed {allowed.reshape(-1)[worst]:.3e} "
                            f"(restatement {e32:.3e}) at flat index {worst}")
    return report, failures
