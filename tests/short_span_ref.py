"""The sets of the tier-5 tests under an ends-free span (test_short_span_cpu.py, test_gpu_short_span_*.py) -- test infrastructure only.

Every set is rebuilt from endsfree_ref.Rng seeds, bit for bit on every machine.  WFA2's gap-affine answers are stored in
tests/golden/endsfree.short_<set>.alg[.gz], one "-score<TAB>CIGAR" line per pair ("*": an empty CIGAR; make_golden_short_span.py writes
them, the sets of thousands of lines gzipped);
the metric sets are answered by linear_endsfree_ref.wfa_linear_endsfree_model when a test runs, computed once and shared (model()).

  sweep   SWEEP_PAIRS pairs of 12-40 bases per penalty set, all under SWEEP_SPAN: every (x, o, e) wfa_short_supported takes and that
          has no common factor, a few that have one (FACTOR_PENS), and every metric wfa_short_lin_supported takes.  Budget: the largest
          under which plan_tier's bound still fits 16 lanes (sweep_budget).
  mixed   MIXED_N shuffled pairs (reads in windows at 0 / 3 / 10 %, unrelated, identical, empty, one base, lengths around the
          packed-word seams, ~1 % with N / IUPAC bytes) under MIXED_CALLS: one span, lanes and budget per call.
  long    LONG_N pairs of 241 / 273 / 497 / 529 bases under LONG_SPAN: the staging tails of a 16-lane group.
  tiny    all 961 ordered pairs of strings over {A, C} of 0-4 bases, and each again with one base replaced by a G, under each of
          TINY_SPANS.

lanes() restates plan_tier's rule (wfa_host.hip); tier5_pairs() restates the retry rule (a failure's budget is four times the last,
at least 16) to say how many pairs finish on tier 5 over a whole call."""
import gzip
import math
import os

import numpy as np

import endsfree_ref as er
import linear_endsfree_ref as ler
import linear_ref as lr

INT_MAX = er.INT_MAX
GOLDEN = er.GOLDEN
ACGT = set(b"ACGT")


def _sub(s, i):
    return s[:i] + bytes([b"ACGT"[(b"ACGT".index(s[i]) + 1) % 4]]) + s[i + 1:]


def is_metric(pen):
    return isinstance(pen[0], str)


def reduced(pen):
    """-> (x or None, o, e, factor): the penalties the kernels run, the common factor divided out (a metric: o = 0, e = g)."""
    if is_metric(pen):
        x, g = lr.pens_of(pen)
        f = g if x is None else math.gcd(x, g)
        return (None if x is None else x // f), 0, g // f, f
    f = math.gcd(*pen)
    return pen[0] // f, pen[1] // f, pen[2] // f, f


def lanes(pen, span, max_error, pairs):
    """plan_tier's rule -> 16 / 32 / 64, or None where the bound does not fit a group: (S - o) / e + 1 diagonals (S the budget without
    the common factor, at least 1) plus the four free-base counts clamped to the batch's longest sequence, never more than every
    diagonal of the longest pair, and one lane to spare."""
    _, o, e, f = reduced(pen)
    m = max(1, max(max(len(p), len(t)) for p, t in pairs))
    s = max(1, max_error // f)
    width = min(2 * m + 1, max(1, (s - o) // e + 1 if s >= o else 1) + sum(min(v, m) for v in span))
    return next((l for l in (16, 32, 64) if width + 1 <= l), None)


def tier5_pairs(pen, span, max_error, pairs, scores):
    """-> (pairs that finish on tier 5 over the whole call, pairs that come back from the first launch): the first launch under
    max_error, every re-run of what failed under four times the budget before (at least 16) while the rule still plans tier 5."""
    f = reduced(pen)[3]
    left = [int(s) for s in scores]
    budget, on5, retried = max(1, max_error // f) * f, 0, None
    while left and lanes(pen, span, budget, pairs) is not None and budget // f <= 30000:
        on5 += sum(1 for s in left if s <= budget)
        left = [s for s in left if s > budget]
        retried = len(left) if retried is None else retried
        budget = max(16, 4 * (budget // f)) * f
    return on5, (len(left) if retried is None else retried)


def raw_pair(p, t):
    return bool(set(p + t) - ACGT)


# ---- sweep ---------------------------------------------------------------------------------------------------------------------
SWEEP_SPAN = (1, 1, 2, 1)
SWEEP_PAIRS = 19
AFFINE_PENS = tuple((x, o, e) for e in range(1, 5) for x in range(1, 9) for o in range(0, 9 - e) if math.gcd(x, o, e) == 1)
FACTOR_PENS = ((4, 6, 2), (6, 3, 3), (8, 4, 4), (2, 0, 2), (6, 2, 4))      # run as (2,3,1), (2,1,1), (2,1,1), (1,0,1), (3,1,2)
METRIC_PENS = (lr.EDIT, lr.INDEL) + tuple(("linear", x, g) for g in range(1, 5) for x in range(1, 9))


def sweep_cap(pen):
    """The largest budget under which SWEEP_SPAN (five free bases) plans 16 lanes: (S - o) / e + 1 + 5 + 1 <= 16."""
    _, o, e, f = reduced(pen)
    return (o + 10 * e - 1) * f


def sweep_budget(pen, scores):
    """sweep_cap, and below the reference's largest score of the set (cheap mismatches under an expensive extension: the unrelated
    pair would fit the cap)."""
    return min(sweep_cap(pen), max(scores) - 1)


def sweep_pairs(pen, index):
    """SWEEP_PAIRS pairs around one read of 18-26 bases; the text leads with the two bases and ends with the one base SWEEP_SPAN frees
    unless said otherwise.  0 identical; 1 a substitution mid-read; 2-4 an insertion and 5-7 a deletion of 1, 2 and D = max(x, o + e)
    bases mid-read; 8-11 a gap of two paid bases that continues the free run at the text's end, the text's begin, the pattern's end,
    the pattern's begin; 12 a substitution in the read's last base; 13 the read against itself; 14 a substitution and a one-base
    insertion; 15 two substitutions; 16, 17 the read at ~6 %; 18 unrelated."""
    x, o, e, _ = reduced(pen)
    rng = er.Rng(20270100 + 1000 * (1 if is_metric(pen) else 0) + index)
    d = max(x or 1, o + e)
    core = rng.seq(rng.integer(18, 27))
    h = len(core) // 2
    lead, tail = rng.seq(2), rng.seq(1)
    pairs = [(core, lead + core + tail), (core, lead + _sub(core, h) + tail)]
    pairs += [(core, lead + core[:h] + rng.seq(n) + core[h:] + tail) for n in (1, 2, d)]
    pairs += [(core, lead + core[:h] + core[h + n:] + tail) for n in (1, 2, d)]
    pairs += [(core, lead + core + rng.seq(1 + 2)), (core, rng.seq(2 + 2) + core + tail), (core + rng.seq(1 + 2), lead + core),
              (rng.seq(1 + 2) + core, core + tail)]
    pairs += [(core, lead + _sub(core, len(core) - 1) + tail), (core, core)]
    pairs += [(core, lead + _sub(core, 4)[:h] + rng.seq(1) + core[h:] + tail), (core, lead + _sub(_sub(core, 5), len(core) - 6) + tail)]
    pairs += [(core, lead + rng.mutate(core, 0.06) + tail) for _ in range(2)]
    pairs.append((rng.seq(24), rng.seq(30)))
    assert len(pairs) == SWEEP_PAIRS and all(12 <= len(s) <= 40 for pair in pairs for s in pair)
    return pairs


def sweep_set(family):
    """-> [(penalties, pairs)] of "affine" (AFFINE_PENS, then FACTOR_PENS) or "metric"."""
    pens = AFFINE_PENS + FACTOR_PENS if family == "affine" else METRIC_PENS
    return [(pen, sweep_pairs(pen, i)) for i, pen in enumerate(pens)]


# ---- mixed ---------------------------------------------------------------------------------------------------------------------
# The smallest counts that give a launch of one wavefront per CU (256 of them) three iterations per wavefront -- 513 work items or more:
# 2051 pairs on 16 lanes (four a wavefront), 1027 on 32 lanes, 515 on 64 -- and are no multiple of four or two, so that the last
# wavefront is partial.  Each call runs that many pairs from the front of the set.
MIXED_N, MIXED_N32, MIXED_N64 = 2051, 1027, 515
MIXED_AFFINE, MIXED_METRIC = ((2, 3, 1), (5, 3, 2)), (lr.EDIT, ("linear", 3, 2))
# (span, lanes, pairs of the set that run, {penalties: budget}) -- budgets from the fixture's scores, within what the lanes allow
MIXED_CALLS = (
    ((0, 0, 8, 8), 32, MIXED_N32, {(2, 3, 1): 17, (5, 3, 2): 30, lr.EDIT: 6, ("linear", 3, 2): 14}),
    ((0, 0, 3, 3), 16, MIXED_N, {(2, 3, 1): 11, (5, 3, 2): 20, lr.EDIT: 8, ("linear", 3, 2): 17}),
    ((0, 0, 16, 16), 64, MIXED_N64, {(2, 3, 1): 10, (5, 3, 2): 20, lr.EDIT: 5, ("linear", 3, 2): 12}),
)
_SEAMS = (15, 16, 17, 31, 32, 33)


def mixed_pairs():
    rng = er.Rng(20270301)
    pairs = []
    for i in range(MIXED_N):
        kind = rng.integer(0, 100)
        if kind < 15:
            p, t = rng.seq(rng.integer(16, 33)), rng.seq(rng.integer(16, 33))
        elif kind < 22:
            p = rng.seq(rng.integer(8, 61))
            t = p
        elif kind < 26:
            s = rng.seq(rng.integer(0, 13))
            p, t = ((b"", s), (s, b""), (b"", b""))[i % 3]
        elif kind < 30:
            s = rng.seq(rng.integer(1, 11))
            p, t = ((s[:1], s), (s, s[:1]), (s[:1], rng.seq(1)))[i % 3]
        else:
            read = rng.seq(_SEAMS[i % 6] if kind < 42 else rng.integer(8, 61))
            rate = (0.0, 0.03, 0.10)[rng.integer(0, 3)]
            p, t = read, rng.seq(rng.integer(0, 9)) + rng.mutate(read, rate) + rng.seq(rng.integer(0, 9))
        if rng.integer(0, 100) == 0 and p and t:
            side, at = rng.integer(0, 3), rng.integer(0, 1 << 16)
            if side != 1:
                p = p[:at % len(p)] + b"NRY"[i % 3:i % 3 + 1] + p[at % len(p) + 1:]
            if side != 0:
                t = t[:at % len(t)] + b"NKW"[i % 3:i % 3 + 1] + t[at % len(t) + 1:]
        pairs.append((p, t))
    order = np.argsort(er.Rng(20270302).u64(MIXED_N), kind="stable")
    return [pairs[j] for j in order]


# ---- long ----------------------------------------------------------------------------------------------------------------------
# A 16-lane group stages a sequence's first 16 words (ASCII: 256 bases) or 32 words (packed: 512 bases) from registers and the rest in
# a loop: 241 and 497 bases are the shortest whose words -- bases / 16 rounded up, plus one of padding -- enter either loop, 273 and 529
# bases put bases into those words.
LONG_N, LONG_SPAN, LONG_LENGTHS = 64, (0, 0, 4, 4), (241, 273, 497, 529)
LONG_BUDGET = {(2, 3, 1): 9, lr.EDIT: 6}      # the largest that plan 16 lanes under LONG_SPAN
LONG_TAIL_PATTERN, LONG_TAIL_TEXT = 0, 1      # pairs whose only edit lies beyond base 512 of the pattern / of the text


def long_pairs():
    rng = er.Rng(20270401)
    p = rng.seq(529)
    pairs = [(_sub(p, 520), rng.seq(2) + p + rng.seq(3))]
    p = rng.seq(529)
    pairs.append((p, rng.seq(4) + p[:517] + rng.seq(1) + p[517:] + rng.seq(1)))
    while len(pairs) < LONG_N:
        i = len(pairs)
        p = rng.seq(LONG_LENGTHS[i % 4])
        t = p
        # two or three planted edits, the last one within the sequence's last 30 bases; every eighth pair: eight (over either budget)
        spots = sorted(rng.integer(10, len(p) - 40) for _ in range(7 if i % 8 == 7 else 1 + i % 2)) + [len(p) - 1 - rng.integer(0, 30)]
        for n, at in enumerate(reversed(spots)):
            if i % 8 != 7 and n == 1 and i % 3 == 0:
                t = t[:at] + t[at + 1:] if i % 2 else t[:at] + rng.seq(1) + t[at:]
            else:
                t = _sub(t, at)
        pairs.append((p, rng.seq(rng.integer(0, 5)) + t + rng.seq(rng.integer(0, 5))))
    return pairs


# ---- tiny ----------------------------------------------------------------------------------------------------------------------
TINY_SPANS = ((INT_MAX, INT_MAX, INT_MAX, INT_MAX), (0, 0, INT_MAX, INT_MAX), (INT_MAX, INT_MAX, 0, 0), (2, 1, 1, 2), (0, 3, 3, 0), (0, 0, 0, 0))
TINY_AFFINE, TINY_METRIC = ((2, 3, 1), (1, 0, 1), (3, 1, 2), (5, 2, 3)), (lr.EDIT, lr.INDEL, ("linear", 3, 2))
TINY_WIDE_SPANS = (TINY_SPANS[0], TINY_SPANS[3])      # run again on 64 lanes
TINY_N = 961 + 960                                    # every ordered pair over {A, C}, and each but the empty one with one G


def tiny_pairs():
    words = [b""]
    for n in range(1, 5):
        words += [bytes(b"AC"[(v >> i) & 1] for i in range(n)) for v in range(1 << n)]
    assert len(words) == 31
    pairs = [(p, t) for p in words for t in words]
    # each again with one base replaced by a G (mismatches against a third letter): in the pattern and in the text by turns, where
    # that sequence has a base, at a position that moves along with the pair's number
    third = []
    for i, (p, t) in enumerate(pairs):
        side = i % 2 if (p, t)[i % 2] else 1 - i % 2
        s = (p, t)[side]
        if s:
            at = (i // 2) % len(s)
            s = s[:at] + b"G" + s[at + 1:]
            third.append((s, t) if side == 0 else (p, s))
    assert len(third) == TINY_N - 961
    return pairs + third


# ---- fixtures and the model ----------------------------------------------------------------------------------------------------
def affine_sets():
    """-> {fixture name: [(penalties, span, pairs)]}: the gap-affine calls whose answers the fixtures hold, in file order."""
    mixed, tiny = mixed_pairs(), tiny_pairs()
    return {
        "short_sweep": [(pen, SWEEP_SPAN, pairs) for pen, pairs in sweep_set("affine")],
        "short_mixed": [(pen, span, mixed[:n]) for span, _, n, _ in MIXED_CALLS for pen in MIXED_AFFINE],
        "short_long": [((2, 3, 1), LONG_SPAN, long_pairs())],
        "short_tiny": [(pen, span, tiny) for pen in TINY_AFFINE for span in TINY_SPANS],
    }


_cache = {}


# The long set's 64 lines are kept as text.  The others hold thousands of generated lines each -- as text well over half a MiB together,
# more than the fixtures of this suite may add -- and are kept as gzip of the same "-score<TAB>CIGAR" text (zcat shows the lines);
# test_short_span_cpu.py pins every line of them to the dynamic program.
ZIPPED = ("short_sweep", "short_mixed", "short_tiny")


def fixture_path(name):
    return os.path.join(GOLDEN, f"endsfree.{name}.alg" + (".gz" if name in ZIPPED else ""))


def write_fixture(name, scores, cigars):
    text = "".join(f"{-int(s)}\t{c or '*'}\n" for s, c in zip(scores, cigars)).encode()
    with open(fixture_path(name), "wb") as f:
        if name in ZIPPED:
            with gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0) as z:      # (no name, no time: the same bytes every run)
                z.write(text)
        else:
            f.write(text)


def read_fixture(name):
    """-> {(penalties, span): [(score, cigar)]} of a gap-affine fixture; read once, shared, not to be changed."""
    if name not in _cache:
        with (gzip.open if name in ZIPPED else open)(fixture_path(name), "rb") as f:
            lines = iter(f.read().decode().splitlines())
        out = {}
        for pen, span, pairs in affine_sets()[name]:
            rows = [next(lines).split("\t") for _ in pairs]
            out[(pen, span)] = [(-int(s), "" if c == "*" else c) for s, c in rows]
        assert next(lines, None) is None
        _cache[name] = out
    return _cache[name]


def model(pen, span, pairs, key):
    """-> [(score, cigar, (k0, k1))] of a metric call from the model; computed once per key, shared, not to be changed.  Pairs that
    clamp the span to the same values and hold the same bytes are computed once."""
    key = (key, pen, span)
    if key not in _cache:
        seen = _cache.setdefault("pairs", {})
        out = []
        for p, t in pairs:
            k = (p, t, pen, er.clamp_span(span, len(p), len(t)))
            if k not in seen:
                seen[k] = ler.wfa_linear_endsfree_model(p, t, pen, span)
            out.append(seen[k])
        _cache[key] = out
    return _cache[key]


# ---- one device call (the GPU tests) ---------------------------------------------------------------------------------------------
INT32_MIN = -(2**31)
_priced = {}


def check_call(al, batch, pairs, pen, span, budget, cigar, ref, tag):
    """One call of a DeviceAligner on an uploaded batch against ref = [(score, cigar[, (k0, k1)])]: every score; k1 inside the pair's
    interval of end diagonals, and the model's under a metric; with CIGARs every byte and (k0, k1) pricing the CIGAR at the score
    (check_cigar with ends=; priced once per pair's bytes, CIGAR and pair of diagonals), without them k0 == INT32_MIN.  -> stats"""
    metric = is_metric(pen)
    s, c, e = al.align(batch, None if metric else pen, max_error=budget, compute_cigar=cigar, span=span, fetch_ends=True,
                       linear=pen if metric else None)
    want = np.array([r[0] for r in ref], dtype=np.int64)
    bad = np.nonzero(np.asarray(s, dtype=np.int64) != want)[0]
    assert bad.size == 0, (tag, "scores", [(int(i), pairs[i], int(s[i]), int(want[i])) for i in bad[:5]])
    kend = np.array([len(t) - len(p) for p, t in pairs], dtype=np.int64)
    cl = np.array([er.clamp_span(span, len(p), len(t)) for p, t in pairs], dtype=np.int64).reshape(-1, 4)
    assert ((kend - cl[:, 3] <= e[:, 1]) & (e[:, 1] <= kend + cl[:, 1])).all(), (tag, "k1 outside the end diagonals")
    if metric:
        assert list(e[:, 1]) == [r[2][1] for r in ref], (tag, "k1")
    if not cigar:
        assert (e[:, 0] == INT32_MIN).all(), (tag, "k0 of a score-only call")
        return al.stats()
    got = ["" if v is None else v for v in c]
    bad = [i for i, (g, r) in enumerate(zip(got, ref)) if g != r[1]]
    assert not bad, (tag, "CIGARs", [(i, pairs[i], got[i], ref[i][1]) for i in bad[:5]])
    if metric:
        assert list(e[:, 0]) == [r[2][0] for r in ref], (tag, "k0")
    for i, ((p, t), r) in enumerate(zip(pairs, ref)):
        key = (pen, span, p, t, r[1], int(e[i][0]), int(e[i][1]))
        if key not in _priced:
            if metric:
                _priced[key] = ler.check_cigar_linear_span(p, t, r[1], pen, span, ends=(int(e[i][0]), int(e[i][1])))
            else:
                _priced[key] = er.check_cigar(p, t, r[1], pen, span, ends=(int(e[i][0]), int(e[i][1])))
        assert _priced[key] == (True, r[0]), (tag, i, p, t, r, list(e[i]))
    return al.stats()
