"""Whisper's batch-decoder rule kernels (csrc/select.hip) against the float64 statement of tests/rules_topk_reference.py on the
designed rows of tests/rules_pick_cases.py, through diagnostic entries that run the production launchers unchanged:
  R  wlk_diag_pick_rows   rules_pick_rows_kernel   (rules_pick_body<true> up to 53 248 entries, <false> beyond)
  O  wlk_diag_pick_one    rules_pick_kernel        (rules_pick_body<false> at every size)
  T  wlk_diag_pick_topk   rules_topk_kernel        (rules_topk_body<true> / <false>), k = 1, 2 and 8
  D  wlk_diag_draft_pick  draft_pick_rows_kernel   (the body as R takes it, the state walked on the device), history cases
and wlk_diag_pick_advance (common.h: pick_rules_advance) against `history_state` over every history of up to 5 tokens.

Ids: equal to float64 in every entry of every case - the cases hold no near-tie that was not planted
(tests/test_rules_pick_cases_cpu.py), exact ties go to the lowest id, the order is (value descending, id ascending), missing
entries are (-inf, -1).  A row with one allowed entry gives the log-probability 0.
Log-probabilities: |got - want| <= max(2 E32, 2e-6) + 2 spacing_fp32(|want|) per entry.  E32 is the worst error the float32
numpy restatement (rules_topk_reference.rules_topk_f32) has against float64 over the case's family - what float32 arithmetic
costs on these rows whoever does it; 2e-6 is what the suite already allows the one-row kernel against the host rules
(tests/test_gpu_window_group.py); the two spacings are the two roundings of (x - max) - log(sum).
Bits: O and R give the same bits on every case (select.hip's contract of the two kernels); each row of a launch of several
gives the bits of that row alone; T at k = 1 names R's token.
A diag call that fails ends the test session (pytest.exit): the device's state is unknown, nothing more is launched.  Figures
go to rules_pick_report.json in the directory WLK_REPORT_DIR names (default: test_reports/)."""
import json
import os

import numpy as np
import pytest

import rules_pick_cases as RC
import rules_topk_reference as REF
from whisperlivekit_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}
FLOOR = 2e-6
KS = (1, 2, 8)


def report(key, value):
    REPORT[key] = value
    out = os.environ.get("WLK_REPORT_DIR") or os.path.join(ROOT, "test_reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "rules_pick_report.json"), "w") as fh:
        json.dump(REPORT, fh, indent=1, sort_keys=True)


def dev(what, fn, *args):
    """a diag call on arguments the entry documents as good: any error ends the session, nothing is retried"""
    try:
        return fn(*args)
    except _lib.WlkError as e:
        pytest.exit(f"{what}: {e}", returncode=3)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_REF = {}


def want(c, mask=None, tag="own"):
    """-> (log-probabilities [8] float64, ids [8], float32 restatement [8]) of a case under its own or another mask; the
    k best of a smaller k are the first k of these.  Computed once."""
    key = (c["name"], tag)
    if key not in _REF:
        m = c["mask"] if mask is None else mask
        lp, ids = REF.rules_topk_reference(c["logits"][None], m, [c["state"]], RC.K_MAX)
        _REF[key] = (lp[0], ids[0], REF.rules_topk_f32(c["logits"][None], m, [c["state"]], ids)[0])
    return _REF[key]


def e32_of(refs):
    worst = 0.0
    for lp, _ids, lp32 in refs:
        fin = np.isfinite(lp)
        assert np.array_equal(np.isfinite(lp32), fin)
        worst = max(worst, float(np.abs(lp32[fin].astype(np.float64) - lp[fin]).max()))
    return worst


def allowance(lp, e32):
    fin = np.where(np.isfinite(lp), lp, 0.0)
    return max(2 * e32, FLOOR) + 2 * np.spacing(np.abs(fin).astype(np.float32)).astype(np.float64)


class Tally:
    """failures and the worst log-probability error per form"""

    def __init__(self, e32):
        self.e32, self.fails, self.err, self.n = e32, [], {}, 0

    def check(self, form, name, got_lp, got_ids, ref):
        """got_lp, got_ids [k] against the first k entries of the float64 result"""
        got_lp, got_ids = np.atleast_1d(got_lp), np.atleast_1d(got_ids)
        k = len(got_ids)
        lp, ids = ref[0][:k], ref[1][:k]
        self.n += k
        if not np.array_equal(got_ids, ids):
            self.fails.append(f"{name} {form}: ids {got_ids.tolist()} for {ids.tolist()}")
            return
        gone = ids < 0
        if not (np.isneginf(got_lp[gone])).all():
            self.fails.append(f"{name} {form}: a missing entry is not -inf")
        err = np.abs(got_lp[~gone].astype(np.float64) - lp[~gone])
        if err.size:
            self.err[form] = max(self.err.get(form, 0.0), float(err.max()))
            tol = allowance(lp[~gone], self.e32)
            if not (err <= tol).all():
                at = int((err - tol).argmax())
                self.fails.append(f"{name} {form}: log-probability {got_lp[~gone][at]!r} for {lp[~gone][at]!r}: off by {err[at]:.3e}, allowed {tol[at]:.3e}")

    def done(self, what):
        rep = dict(e32=self.e32, entries=self.n, device_err=self.err)
        print(what, json.dumps(rep))
        report(what, rep)
        assert not self.fails, f"{len(self.fails)} failures:\n" + "\n".join(self.fails[:40])


def draft_of(c):
    """the draft whose position len(history) is the case: (draft tokens, position)"""
    h = c["history"]
    return (h, len(h)) if h else ([c["state"]["timestamp_begin"]], 0)


# ---- every single-row case through the four forms -------------------------------------------------------------------------------
@pytest.mark.parametrize("family", RC.FAMILIES)
def test_every_case_through_every_form(family):
    from whisperlivekit_amd.engine import draft_pick, pick_one, pick_rows, pick_topk_rows
    cases = [c for c in RC.single_cases() if c["family"] == family]
    t = Tally(e32_of([want(c) for c in cases]))
    sizes = set()
    for c in cases:
        ref, x, name = want(c), c["logits"][None], c["name"]
        sizes.add(c["V"])
        r_tok, r_lp = dev(f"wlk_diag_pick_rows ({name})", pick_rows, x, c["mask"][None], [0], [c["state"]])
        t.check("R", name, r_lp, r_tok, ref)
        o_tok, o_lp = dev(f"wlk_diag_pick_one ({name})", pick_one, x[0], c["mask"], c["state"])
        t.check("O", name, o_lp, o_tok, ref)
        if (o_tok, bits(o_lp)[0]) != (int(r_tok[0]), bits(r_lp)[0]):
            t.fails.append(f"{name}: the one-row kernel gives ({o_tok}, {o_lp!r}), the rows kernel ({r_tok[0]}, {r_lp[0]!r})")
        for k in KS:
            lp, ids = dev(f"wlk_diag_pick_topk ({name}, k {k})", pick_topk_rows, x, c["mask"], [c["state"]], k)
            t.check(f"T{k}", name, lp[0], ids[0], ref)
            if c.get("single") and float(lp[0, 0]) != 0.0:
                t.fails.append(f"{name} T{k}: the only allowed entry has log-probability {lp[0, 0]!r}")
            if k == 1 and int(ids[0, 0]) != int(r_tok[0]):
                t.fails.append(f"{name}: the top-1 is {ids[0, 0]}, the pick {r_tok[0]}")
        if c.get("single"):
            for form, v in (("R", r_lp[0]), ("O", o_lp)):
                if float(v) != 0.0:
                    t.fails.append(f"{name} {form}: the only allowed entry has log-probability {v!r}")
        if "history" in c:
            draft, pos = draft_of(c)
            first = RC.state_after(c["V"], [], max_initial=c["state"]["max_initial"])
            d_tok, d_lp, _res = dev(f"wlk_diag_draft_pick ({name})", draft_pick, np.repeat(x, len(draft) + 1, axis=0), c["mask"],
                                    first, draft)
            t.check("D", name, d_lp[pos], d_tok[pos], ref)
            if (int(d_tok[pos]), bits(d_lp)[pos]) != (int(r_tok[0]), bits(r_lp)[0]):
                t.fails.append(f"{name}: the draft kernel's position {pos} differs from the rows kernel")
    assert {RC.REGS_LAST, RC.MEM_FIRST} <= sizes or family in ("borders", "degenerate")
    assert RC.MEM_FIRST in sizes                                   # both forms of either body ran
    t.done(family)


# ---- several rows in one launch -------------------------------------------------------------------------------------------------
def test_rows_of_one_launch_are_the_rows_alone():
    from whisperlivekit_amd.engine import pick_rows, pick_topk_rows
    groups = RC.row_groups()
    t = Tally(e32_of([want(c) for g in groups for c in g["rows"]] + [want(c, g["shared"], "shared") for g in groups for c in g["rows"]]))
    for g in groups:
        rows, name = g["rows"], g["name"]
        x = np.stack([c["logits"] for c in rows])
        states = [c["state"] for c in rows]
        masks, index = RC.stack_masks(rows)
        toks, lps = dev(f"wlk_diag_pick_rows ({name})", pick_rows, x, masks, index, states)
        for r, c in enumerate(rows):
            t.check("R", f"{name}[{r}]", lps[r], toks[r], want(c))
            a_tok, a_lp = dev(f"wlk_diag_pick_rows ({name}, row {r} alone)", pick_rows, x[r:r + 1], c["mask"][None], [0], [c["state"]])
            if (int(a_tok[0]), bits(a_lp)[0]) != (int(toks[r]), bits(lps)[r]):
                t.fails.append(f"{name}: row {r} of the launch differs from the row alone")
        for k in KS:
            lp, ids = dev(f"wlk_diag_pick_topk ({name}, k {k})", pick_topk_rows, x, g["shared"], states, k)
            for r, c in enumerate(rows):
                t.check(f"T{k}", f"{name}[{r}]", lp[r], ids[r], want(c, g["shared"], "shared"))
                a_lp, a_ids = dev(f"wlk_diag_pick_topk ({name}, row {r} alone, k {k})", pick_topk_rows, x[r:r + 1], g["shared"],
                                  [c["state"]], k)
                if not (np.array_equal(a_ids[0], ids[r]) and np.array_equal(bits(a_lp[0]), bits(lp[r]))):
                    t.fails.append(f"{name}: row {r} of the top-{k} launch differs from the row alone")
    t.done("rows")


# ---- the transition -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("without_timestamps", [0, 1])
@pytest.mark.parametrize("max_initial", [0, -1])
def test_the_device_transition_is_the_state_of_the_longer_history(max_initial, without_timestamps):
    from whisperlivekit_amd.engine import pick_advance
    levels = RC.walk_levels()
    states = {(): RC.walk_state((), max_initial, without_timestamps)}     # the DEVICE's state after every prefix
    assert states[()]["first_step"] == 1
    for level in levels[1:]:                                               # one launch per length
        got = dev(f"wlk_diag_pick_advance (length {len(level[0])})", pick_advance, [states[h[:-1]] for h in level], [h[-1] for h in level])
        for h, g in zip(level, got):
            assert g == RC.walk_state(h, max_initial, without_timestamps), (h, g)
            states[h] = g
    assert len(states) == sum(len(RC.WALK_ALPHABET) ** n for n in range(RC.WALK_LEN + 1))
    assert {(s["ts_mode"], s["ts_bound"] - RC.WALK_TB) for s in states.values()} >= {(0, 0), (1, 1), (2, 0), (2, 5), (1, 6), (0, 6)}


# ---- drafts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", RC.DRAFT_SIZES)
def test_every_position_of_a_draft_and_what_is_accepted(V):
    from whisperlivekit_amd.engine import draft_pick
    mask = RC.base_mask(V)
    histories = [RC.draft_history(V, i) for i in range(3)]
    logits = RC.draft_logits(V, histories)
    first = RC.state_after(V, [])
    refs, runs = {}, []

    def ref_of(i, j, st):
        key = (i, j, tuple(sorted(st.items())))
        if key not in refs:
            lp, ids = REF.rules_topk_reference(logits[i][j][None], mask, [st], 1)
            assert not REF.unplanted_near_ties(logits[i][j][None], mask, [st], 1).any(), key
            refs[key] = (lp[0], ids[0], REF.rules_topk_f32(logits[i][j][None], mask, [st], ids)[0])
        return refs[key]
    for i, h in enumerate(histories):
        for m in RC.DRAFT_MISMATCH:
            draft = list(h)
            if m is not None:
                draft[m] = RC.other_token(V, h, m)
            runs.append((i, m, draft, [ref_of(i, j, RC.state_after(V, draft[:j])) for j in range(RC.DRAFT_LEN + 1)]))
    t = Tally(e32_of(list(refs.values())))
    for i, m, draft, ref in runs:
        name = f"draft/v{V}/h{i}/mismatch_{m}"
        toks, lps, res = dev(f"wlk_diag_draft_pick ({name})", draft_pick, logits[i], mask, first, draft)
        for j in range(RC.DRAFT_LEN + 1):
            t.check("D", f"{name}[{j}]", lps[j], toks[j], ref[j])
        picks = [int(r[1][0]) for r in ref]
        miss = [j for j in range(RC.DRAFT_LEN) if picks[j] != draft[j]]
        accepted = miss[0] if miss else RC.DRAFT_LEN
        assert accepted == (RC.DRAFT_LEN if m is None else m), (name, accepted)
        if (res["accepted"], res["next_token"]) != (accepted, picks[accepted]):
            t.fails.append(f"{name}: accepted {res['accepted']}, next {res['next_token']} for {accepted}, {picks[accepted]}")
        elif bits(res["next_logprob"])[0] != bits(lps)[accepted]:
            t.fails.append(f"{name}: the next token's log-probability is not that of position {accepted}")
        total = np.float32(0)
        for j in range(accepted + 1):
            total = np.float32(total + lps[j])
        if bits(res["sum_logprob"])[0] != bits(total)[0]:
            t.fails.append(f"{name}: sum {res['sum_logprob']!r} for {total!r}")
    t.done(f"draft_v{V}")
