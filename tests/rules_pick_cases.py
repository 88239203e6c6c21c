"""Designed logits rows for whisper's batch-decoder rule kernels (csrc/select.hip: rules_pick_kernel, rules_pick_rows_kernel,
draft_pick_rows_kernel, rules_topk_kernel; common.h: pick_rules_advance) - TEST infrastructure only, shared by
tests/test_rules_pick_cases_cpu.py and tests/test_gpu_rules_pick.py.  No model, no tokenizer: a case is a logits row, a rule
mask and a wlk_pick_params block, built from a seed that is derived from the case's name.

Families:
  margin      one text entry planted so that logsumexp(allowed timestamps) - max(allowed text) is a chosen margin, in pairs of
              opposite sign on the same draw: the timestamps win one, the planted text token the other.
  ties        bit-equal float32 maxima at chosen index pairs (neighbours, across a wave, across the 1024-entry stride of a
              thread, text with text, timestamp with timestamp), a triple in three waves, and pairs whose lower id the rules
              forbid.  Every other gap in the ranking is >= 1e-3.
  borders     per rule, the token on either side of its border holds the two largest logits of the row, the forbidden one
              the larger; a comparison that is off by one picks another token.
  degenerate  one allowed entry, only timestamps, only text, -inf among the allowed entries, fewer allowed entries than k,
              all logits equal, row maxima of +80 and -100.
  random      normal logits of scale 3 under the 12 histories of the existing rule tests.
  rows        1, 2, 3, 5 and 8 of the rows above in one launch, with different parameter blocks and (for the rows pick)
              different masks.
A case is drawn again, with a counter in its seed, until the float64 reference sees no near-tie (rules_topk_reference.
near_ties at 1e-4; 1e-3 for `ties`) other than the planted exact ties: the GPU test compares every id, no case is exempt.

Layout of a vocabulary of V entries: timestamp_begin = V - 1501 (the 1501 timestamps of every Whisper vocabulary) for the
sizes that have room for it; V // 2 for 1023..1025, 4 for V = 7.  <|endoftext|> = tb - 107 and <|notimestamps|> = tb - 1 as in
the multilingual vocabulary (3 and none for V = 7)."""
import zlib

import numpy as np

import rules_topk_reference as REF

SIZES = (7, 1023, 1024, 1025, 51864, 51865, 51866, 53248, 53249, 60000)
REGS_LAST, MEM_FIRST = 53248, 53249          # kRulesKeep * 1024 and the first row that takes the memory form
K_MAX = 8
FIELDS = ("first_step", "without_timestamps", "timestamp_begin", "eot", "no_timestamps", "ts_mode", "ts_bound", "max_initial")


def layout(V):
    """-> dict(tb, eot, nt, suppressed, blank) of a vocabulary of V entries"""
    if V == 7:
        return dict(tb=4, eot=3, nt=-1, suppressed=(1,), blank=(0, 3))
    tb = V - 1501 if V > 3002 else V // 2
    eot = tb - 107
    return dict(tb=tb, eot=eot, nt=tb - 1, suppressed=(1, 2, 300, 399, tb - 50), blank=(220, eot))


def base_mask(V):
    lay = layout(V)
    return REF.rules_mask(V, lay["suppressed"], lay["blank"])


def state(V, **kw):
    lay = layout(V)
    st = dict(first_step=0, without_timestamps=0, timestamp_begin=lay["tb"], eot=lay["eot"], no_timestamps=lay["nt"], ts_mode=0,
              ts_bound=lay["tb"], max_initial=50)
    st.update(kw)
    assert set(st) == set(FIELDS)
    return st


def rng_of(name, attempt):
    return np.random.default_rng([zlib.crc32(name.encode()), attempt])


def draw(rng, V, scale):
    return (rng.standard_normal(V, dtype=np.float32) * np.float32(scale)).astype(np.float32)


def lse64(x):
    x = np.asarray(x, np.float64)
    m = x.max()
    return m + np.log(np.exp(x - m).sum())


def clean(logits, mask, st, eps=REF.NEAR_TIE):
    """no near-tie that was not planted, for the k = 8 best (which contain those of every smaller k) and the decision"""
    return not REF.unplanted_near_ties(logits[None], mask, [st], K_MAX, eps).any()


def redrawn(name, build, eps=REF.NEAR_TIE):
    """build(rng) -> [case dictionaries] or None; drawn again until every case of the list is clean"""
    for attempt in range(64):
        cases = build(rng_of(name, attempt))
        if cases and all(clean(c["logits"], c["mask"], c["state"], eps) for c in cases):
            for c in cases:
                c["attempt"] = attempt
            return cases
    raise AssertionError(f"{name}: no clean draw in 64 attempts")


def case(name, family, logits, mask, st, **meta):
    assert logits.dtype == np.float32 and mask.dtype == np.uint8 and logits.shape == mask.shape
    assert REF.allowed(mask, st, logits.shape[0]).any(), name       # a row that allows nothing is outside the contract
    return dict(name=name, family=family, V=int(logits.shape[0]), logits=logits, mask=mask, state=st, **meta)


# ---- margin -------------------------------------------------------------------------------------------------------------------
MARGINS = (1e-2, 1e-3, 3.0)
SCALES = (1, 3, 20)


def margin_pair(V, scale, margin):
    """the same draw with the planted text entry at logsumexp(timestamps) -/+ margin"""
    name = f"margin/v{V}/s{scale}/m{margin:g}"
    lay, mask = layout(V), base_mask(V)
    tb = lay["tb"]
    st = state(V, ts_bound=tb + (1 if V == 7 else 2)) if (V // 7 + scale) % 2 else state(V)

    def build(rng):
        x = draw(rng, V, scale)
        ok = REF.allowed(mask, st, V)
        text_ok = np.flatnonzero(ok[:tb])
        plant = int(text_ok[rng.integers(len(text_ok))])
        lse_ts = lse64(x[tb:][ok[tb:]])
        out = []
        for sign in (+1, -1):
            y = x.copy()
            y[plant] = np.float32(lse_ts - sign * margin)
            others = text_ok[text_ok != plant]
            over = float(y[others].max()) - (float(y[plant]) - 1.0) if len(others) else 0.0
            if over > 0:                          # every other text entry at least 1 below the planted one: shifted, not clamped
                y[others] -= np.float32(over + 1e-3)
            got = lse_ts - float(y[:tb][ok[:tb]].max())
            assert abs(got - sign * margin) <= 1e-4 * margin + 4 * np.spacing(np.float32(abs(lse_ts))), (name, got)
            _lp, ids, m, _vals = REF._row(y, mask, st, 1)
            assert abs(m - abs(got)) < 1e-12
            out.append(case(f"{name}/{'ts' if sign > 0 else 'text'}", "margin", y, mask, st, plant=plant, sign=sign, margin=sign * margin))
        return out
    return redrawn(name, build)


# ---- ties ---------------------------------------------------------------------------------------------------------------------
TIE_SIZES = (7, 1025, 51865, REGS_LAST, MEM_FIRST, 60000)


def tie_sets(V):
    """-> [(label, indices with bit-equal maxima, overrides of the state)]; the winner is the lowest ALLOWED index"""
    lay = layout(V)
    tb = lay["tb"]
    sets = [("5_6", (5, 6), {}), ("63_64", (63, 64), {}), ("100_1124", (100, 1124), {}), ("1023_1024", (1023, 1024), {}),
            ("7_tbm1", (7, tb - 1), dict(no_timestamps=-1)), ("tb_tbp1", (tb, tb + 1), {}), ("last_two", (V - 2, V - 1), {}),
            ("three_waves", (10, 70 + (1024 if V > 1100 else 0), 200 + (2048 if V > 2300 else 0)), {}),
            ("lower_masked", (lay["suppressed"][-1], lay["suppressed"][-1] + 1), {}),
            ("lower_bounded", (tb + 1, tb + 2), dict(ts_bound=tb + 2))]
    return [(label, idx, over) for label, idx, over in sets if max(idx) < V and len(set(idx)) == len(idx)]


def tie_case(V, label, idx, over):
    name = f"ties/v{V}/{label}"
    lay, mask = layout(V), base_mask(V)
    tb = lay["tb"]
    st = state(V, **over)

    def build(rng):
        x = draw(rng, V, 3)
        ok = REF.allowed(mask, st, V)
        live = [i for i in idx if ok[i]]
        if label.startswith("lower_"):
            assert live == list(idx[1:]), (name, live)
        else:
            assert live == list(idx), (name, live)
        rest = ok.copy()
        rest[list(idx)] = False
        top = float(x[rest].max())
        if all(i >= tb for i in idx):
            value = top + 3.0                     # timestamps: their group outweighs every text entry anyway
        else:
            value = max(top, lse64(np.append(x[tb:][rest[tb:]], [x[i] for i in live if i >= tb]))) + 3.0     # text that beats the timestamps' sum
        x[list(idx)] = np.float32(value)
        assert len({x[i].tobytes() for i in idx}) == 1
        return [case(name, "ties", x, mask, st, tied=tuple(idx), winner=min(live))]
    return redrawn(name, build, eps=1e-3)[0]


# ---- borders ------------------------------------------------------------------------------------------------------------------
BORDER_SIZES = (7, 1024, 51865, MEM_FIRST)


def border_specs(V):
    """-> [(label, state, [(token, height above the rest of the row)], winner)]: the first plant is the row's raw arg-max"""
    lay = layout(V)
    tb, eot, nt, s, b = lay["tb"], lay["eot"], lay["nt"], lay["suppressed"][-1], lay["blank"][-1]
    text = 5 if V > 7 else 2                      # an allowed text token away from every border
    out = [("mask0_up", state(V), [(s, 12), (s + 1, 10)], s + 1),
           ("mask1_first", state(V, first_step=1, without_timestamps=1), [(b, 12), (b + 1, 10)], b + 1),
           ("mask1_later", state(V, without_timestamps=1), [(b, 12), (b + 1, 10)], b),
           ("mode1", state(V, ts_mode=1, ts_bound=tb + 1, no_timestamps=-1), [(tb, 12), (tb - 1, 10)], tb - 1),
           ("mode2", state(V, ts_mode=2, ts_bound=tb + 1), [(eot - 1, 12), (eot, 10)], eot),
           ("bound_tb", state(V), [(tb, 12), (tb + 1, 10)], tb),
           ("bound_mid", state(V, ts_bound=tb + 2), [(tb + 1, 12), (tb + 2, 10)], tb + 2),
           ("bound_v", state(V, ts_bound=V), [(V - 1, 12), (V - 2, 11), (text, 10)], text),
           ("first_tb", state(V, first_step=1, no_timestamps=-1), [(tb - 1, 12), (tb, 10)], tb),
           ("initial0", state(V, first_step=1, max_initial=0), [(tb + 1, 12), (tb, 10)], tb),
           ("initial50", state(V, first_step=1, max_initial=50), [(tb + 51, 12), (tb + 50, 10)], tb + 50),
           ("initial_none", state(V, first_step=1, max_initial=-1), [(V - 1, 12), (V - 2, 10)], V - 1),
           ("without", state(V, without_timestamps=1, ts_mode=1, ts_bound=V), [(tb, 12), (max(nt, tb - 1), 10)], tb),
           # and no timestamps-versus-text decision: a text entry 1 above the row, below the sum of 1501 timestamps
           ("without_sum", state(V, without_timestamps=1), [(text, 1)], text)]
    if s - 1 not in lay["suppressed"] and s - 1 not in lay["blank"]:
        out.append(("mask0_down", state(V), [(s, 12), (s - 1, 10)], s - 1))
    if nt >= 0:
        out += [("nt_set_down", state(V), [(nt, 12), (nt - 1, 10)], nt - 1), ("nt_set_up", state(V), [(nt, 12), (nt + 1, 10)], nt + 1),
                ("nt_none", state(V, no_timestamps=-1), [(nt, 12), (nt - 1, 10)], nt)]
    return [spec for spec in out if all(0 <= t < V for t, _h in spec[2])]


def border_case(V, label, st, plants, winner):
    name = f"borders/v{V}/{label}"
    mask = base_mask(V)

    def build(rng):
        x = draw(rng, V, 3)
        top = float(x.max())
        for t, h in plants:
            x[t] = np.float32(top + h)            # 10 and more above everything: above the logsumexp of any 1501 of them too
        return [case(name, "borders", x, mask, st, top=plants[0][0], winner=winner)]
    return redrawn(name, build)[0]


# ---- degenerate ---------------------------------------------------------------------------------------------------------------
DEGENERATE_SIZES = (7, 1025, 51865, MEM_FIRST)


def degenerate_cases(V):
    lay, mask = layout(V), base_mask(V)
    tb, text = lay["tb"], (5 if V > 7 else 2)
    out = []

    def add(label, make, eps=REF.NEAR_TIE):
        name = f"degenerate/v{V}/{label}"

        def build(rng):
            x, m, st, meta = make(rng)
            return [case(name, "degenerate", x, m, st, **meta)]
        out.extend(redrawn(name, build, eps))

    def only(ids):
        m = np.ones(V, np.uint8)
        m[list(ids)] = 0
        return m
    add("one_text", lambda rng: (draw(rng, V, 3), only([text]), state(V), dict(winner=text, single=True)))
    add("one_timestamp", lambda rng: (draw(rng, V, 3), only([V - 1]), state(V), dict(winner=V - 1, single=True)))
    add("only_timestamps", lambda rng: (draw(rng, V, 3), mask, state(V, timestamp_begin=0, eot=0, no_timestamps=-1, ts_bound=0), {}))
    add("only_text_tb_v", lambda rng: (draw(rng, V, 3), mask, state(V, timestamp_begin=V, ts_bound=V), {}))
    add("only_text_mode1", lambda rng: (draw(rng, V, 3), mask, state(V, ts_mode=1, ts_bound=tb + 1), {}))

    def holes(rng, where):
        x = draw(rng, V, 3)
        st = state(V)
        ok = np.flatnonzero(REF.allowed(mask, st, V))
        if where == "some":
            pick = rng.choice(ok, size=min(500, len(ok) // 2), replace=False)
        else:
            pick = ok[ok >= tb] if where == "timestamps" else ok[ok < tb]
        x[pick] = -np.inf
        return x, mask, st, dict(holes=len(pick))
    add("inf_some", lambda rng: holes(rng, "some"))
    add("inf_timestamps", lambda rng: holes(rng, "timestamps"))     # the timestamps' group has nothing finite: text decides
    add("inf_text", lambda rng: holes(rng, "text"))
    # fewer allowed entries than k: two text entries and a timestamp, the text entry on top and the timestamp on top
    add("few_text_wins", lambda rng: (np.where(np.arange(V) == text, np.float32(9), draw(rng, V, 3)), only([0 if V > 7 else 2, text, V - 1]),
                                      state(V), {}))
    add("few_timestamp_wins", lambda rng: (np.where(np.arange(V) == V - 1, np.float32(9), draw(rng, V, 3)),
                                           only([0 if V > 7 else 2, text, V - 1]), state(V), {}))
    add("all_equal", lambda rng: (np.full(V, 1.5, np.float32), mask, state(V), dict(equal=True)))

    def shifted(rng, peak):
        x = draw(rng, V, 3)
        x = (x - x.max() + np.float32(peak)).astype(np.float32)
        assert x.max() == np.float32(peak)
        return x, mask, state(V), dict(peak=peak)
    add("max_plus80", lambda rng: shifted(rng, 80.0))
    add("max_minus100", lambda rng: shifted(rng, -100.0))
    return out


# ---- random: the 12 histories of the existing rule tests ------------------------------------------------------------------------
RANDOM_SIZES = (51864, 51865, 51866, REGS_LAST, MEM_FIRST, 60000)


def histories(V, rng):
    lay = layout(V)
    tb, eot = lay["tb"], lay["eot"]
    text = lambda n: [int(t) for t in rng.integers(400, 20000, n)]
    return [[], [tb], [tb + 3], [tb, *text(3)], [tb, *text(2), tb + 40], [tb, *text(2), tb + 40, tb + 40],
            [tb, *text(1), tb + 40, tb + 40, *text(2)], [tb, *text(4), tb + 1499], [tb, *text(2), tb + 700, tb + 700, eot],
            text(5), [tb + 1500], [tb, *text(2), tb + 1500, tb + 1500]]


def state_after(V, history, max_initial=50, without_timestamps=0):
    lay = layout(V)
    return REF.history_state(history, lay["tb"], lay["eot"], lay["nt"], max_initial, without_timestamps)


def random_cases(V):
    mask = base_mask(V)
    out = []
    for i, h in enumerate(histories(V, rng_of(f"random/v{V}/histories", 0))):
        st = state_after(V, h, max_initial=50 if i % 2 == 0 else -1)
        name = f"random/v{V}/h{i}"
        out.extend(redrawn(name, lambda rng: [case(name, "random", draw(rng, V, 3), mask, st, history=list(h))]))
    return out


# ---- every single-row case, built once -----------------------------------------------------------------------------------------
_CACHE = {}


def single_cases():
    if "single" not in _CACHE:
        out = []
        for V in SIZES:
            for scale in SCALES:
                for m in MARGINS:
                    out.extend(margin_pair(V, scale, m))
        for V in TIE_SIZES:
            out.extend(tie_case(V, *spec) for spec in tie_sets(V))
        for V in BORDER_SIZES:
            out.extend(border_case(V, *spec) for spec in border_specs(V))
        for V in DEGENERATE_SIZES:
            out.extend(degenerate_cases(V))
        for V in RANDOM_SIZES:
            out.extend(random_cases(V))
        assert len({c["name"] for c in out}) == len(out)
        _CACHE["single"] = out
    return _CACHE["single"]


def by_name():
    return {c["name"]: c for c in single_cases()}


FAMILIES = ("margin", "ties", "borders", "degenerate", "random")


# ---- rows ---------------------------------------------------------------------------------------------------------------------
ROW_COUNTS = (1, 2, 3, 5, 8)
ROW_SIZES = (7, 51865, MEM_FIRST)


def row_groups():
    """-> [dict(name, V, rows = [single cases], shared = the mask of the top-k launch)]: the rows of one launch carry different
    parameter blocks and, for the rows pick, different masks; the top-k takes one mask, under which every row is clean too
    (a group whose rows are not is passed over for the next selection)."""
    if "rows" in _CACHE:
        return _CACHE["rows"]
    out = []
    for V in ROW_SIZES:
        pool = [c for c in single_cases() if c["V"] == V and not c.get("single") and "few_" not in c["name"]]
        shared = base_mask(V)
        pool = [c for c in pool if REF.allowed(shared, c["state"], V).any() and clean(c["logits"], shared, c["state"])]
        special = [c for c in single_cases() if c["V"] == V and (c.get("single") or "few_" in c["name"])]     # masks of their own
        special = [c for c in special if clean(c["logits"], shared, c["state"])]
        assert len(special) >= 2 and len(pool) >= 8
        for n in ROW_COUNTS:
            key = lambda c: tuple(sorted(c["state"].items()))
            order = [pool[i] for i in rng_of(f"rows/v{V}/n{n}", 0).permutation(len(pool))]
            own = ([special[n % len(special)]] if n >= 2 else []) + ([special[(n + 1) % len(special)]] if n >= 5 else [])
            rows, seen = [], {key(c) for c in own}
            for c in order + order:                # rows under parameter blocks not taken yet first, then whatever is left
                fresh = key(c) not in seen or len(seen) >= len({key(d) for d in pool})
                if len(rows) < n - len(own) and fresh and not any(c is d for d in rows):
                    rows.append(c)
                    seen.add(key(c))
            for at, c in zip((1, 4), own):         # the rows with a mask of their own go second and fifth
                rows.insert(at, c)
            states = [key(c) for c in rows]
            assert len(rows) == n and len(set(states)) >= min(n, 2), (V, n)
            assert n == 1 or len(stack_masks(rows)[1]) == n and len(set(stack_masks(rows)[1])) > 1
            out.append(dict(name=f"rows/v{V}/n{n}", V=V, rows=rows, shared=shared))
    _CACHE["rows"] = out
    return out


def stack_masks(rows):
    """-> (masks [n_masks, V], mask_of_row) with equal masks stored once"""
    masks, index = [], []
    for c in rows:
        for i, m in enumerate(masks):
            if m is c["mask"] or np.array_equal(m, c["mask"]):
                index.append(i)
                break
        else:
            masks.append(c["mask"])
            index.append(len(masks) - 1)
    return np.stack(masks), index


# ---- the transition: every history over a small alphabet -----------------------------------------------------------------------
WALK_V, WALK_TB, WALK_EOT, WALK_LEN = 16, 10, 8, 5
# two text ids, <|endoftext|>, tb, tb + 1, tb + 5 and V - 1 - which at V = 16 and tb = 10 is tb + 5 again: six tokens
WALK_ALPHABET = tuple(sorted({1, 3, WALK_EOT, WALK_TB, WALK_TB + 1, WALK_TB + 5, WALK_V - 1}))


def walk_state(history, max_initial, without_timestamps):
    return REF.history_state(history, WALK_TB, WALK_EOT, WALK_TB - 1, max_initial, without_timestamps)


def walk_levels():
    """-> [[history tuples of length n] for n = 0 .. WALK_LEN]: every sequence over the alphabet, whether the rules would have
    allowed it or not (the transition is a function of the state and the token alone)"""
    levels = [[()]]
    for _ in range(WALK_LEN):
        levels.append([h + (t,) for h in levels[-1] for t in WALK_ALPHABET])
    return levels


# ---- drafts -------------------------------------------------------------------------------------------------------------------
DRAFT_LEN = 200
DRAFT_SIZES = (51865, MEM_FIRST)
DRAFT_MISMATCH = (0, 63, 64, 199, None)


def draft_history(V, seed):
    """a history of DRAFT_LEN tokens that obeys the rules from the first step on: text runs, closed timestamp pairs, single
    timestamps followed by text at or above <|endoftext|>"""
    lay, mask = layout(V), base_mask(V)
    tb, eot = lay["tb"], lay["eot"]
    rng = rng_of(f"draft/history{seed}", 0)
    h = [tb + 1]
    while len(h) < DRAFT_LEN:
        st = state_after(V, h)
        ok = REF.allowed(mask, st, V)
        bound = max(st["ts_bound"], tb)
        kinds = []
        if st["ts_mode"] != 1 and bound + 3 < V:
            kinds += ["stamp", "stamp_again"] if st["ts_mode"] == 2 else ["stamp"]
        if st["ts_mode"] == 2:
            kinds.append("high_text")
        else:
            kinds += ["text", "text", "text"]
        if len(h) in (63, 64, 199):               # where the tests plant a mismatch: a text token (its stand-in leaves the states alone)
            kinds = [k for k in kinds if "text" in k]
        kind = kinds[int(rng.integers(len(kinds)))]
        if kind == "stamp":
            t = bound + int(rng.integers(0, 3))
        elif kind == "stamp_again":
            t = bound                             # closes the pair at the stamp that opened it
        elif kind == "high_text":
            t = int(rng.integers(eot + 1, tb - 1))
        else:
            t = int(rng.integers(400, 20000))
        if ok[t] and t != eot:
            h.append(t)
    return h


def other_token(V, h, j):
    """a token of the same kind as h[j] that the state of h[:j] allows and that is not h[j]"""
    lay, mask = layout(V), base_mask(V)
    ok = REF.allowed(mask, state_after(V, h[:j]), V)
    step = -1 if h[j] >= lay["tb"] else 1        # a lower timestamp: every later token of the history stays allowed
    t = h[j] + step
    while not ok[t] or t == lay["eot"] or (t >= lay["tb"]) != (h[j] >= lay["tb"]):
        t += step
    return t


def decoys(st, V):
    """tokens the state forbids and a neighbouring state allows: they hold the row's largest logits"""
    tb = st["timestamp_begin"]
    out = []
    if st["ts_bound"] > tb:
        out.append(st["ts_bound"] - 1)
    if st["ts_mode"] == 1:
        out.append(V - 1)
    if st["ts_mode"] == 2:
        out.append(7)
    if st["first_step"]:
        out += [7, tb + st["max_initial"] + 1]
    return out


def draft_logits(V, histories_):
    """-> {history index: logits [DRAFT_LEN + 1, V]}: one normal draw of scale 3 shared by the histories; row j of history i
    has h[j] planted 10 above the row (the pick follows the history; the last row is left to the draw) and the decoys of
    its state 12 above it."""
    if ("draft", V) in _CACHE:
        return _CACHE[("draft", V)]
    mask = base_mask(V)
    rng = rng_of(f"draft/v{V}/logits", 0)
    base = rng.standard_normal((DRAFT_LEN + 1, V), dtype=np.float32) * np.float32(3)
    top = base.max(axis=1)
    out = {}
    for i, h in enumerate(histories_):
        x = base.copy()
        for j in range(DRAFT_LEN + 1):
            st = state_after(V, h[:j])
            for t in decoys(st, V):
                x[j, t] = top[j] + np.float32(12)
            if j < DRAFT_LEN:
                x[j, h[j]] = top[j] + np.float32(10)
            else:                                 # the free row: drawn again while float64 sees a near-tie in it
                while not clean(x[j], mask, st):
                    x[j] = draw(rng, V, 3)
                    for t in decoys(st, V):
                        x[j, t] = x[j].max() + np.float32(12)
        out[i] = x
    _CACHE[("draft", V)] = out
    return out
