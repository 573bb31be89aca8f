"""Ground truth for ends-free (semi-global) alignment -- test infrastructure only.

  wfa2_endsfree      WFA2 itself, through the reference library that oracle/Makefile compiles in place (oracle/_ref/libwfa2ref.so,
                     optional): wavefront_aligner_set_alignment_free_ends on the aligner behind a ref_new() handle, then ref_run()
  dp_endsfree_score  a plain gap-affine dynamic program with free borders (numpy, one vector step per row)
  check_cigar        validity of a CIGAR that covers both whole sequences, and its cost without the free runs
  make_set / read_golden   the golden sets: pairs rebuilt by a deterministic recipe, WFA2's answers in tests/golden/endsfree.<set>.alg

A span is (pattern_begin_free, pattern_end_free, text_begin_free, text_end_free); every value is clamped to the length of its sequence
pair by pair (WFA2 rejects larger ones)."""
import ctypes as C
import math
import os
import re

import numpy as np

import oracle_lib

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
INT_MAX = 2**31 - 1
SETS = ("small", "wide", "ties")
# one more .alg over the pairs of `small`: ALL of them under one span and one set of penalties -- what a whole batch of a
# launch_alignments* call, a command line or a big tiled batch runs under
ONE_SPAN_SET, ONE_SPAN, ONE_SPAN_PEN = "small_t50", (0, 0, 50, 50), (2, 3, 1)


def clamp_span(span, plen, tlen):
    pb, pe, tb, te = span
    return (min(pb, plen), min(pe, plen), min(tb, tlen), min(te, tlen))


class Wfa2EndsFree:
    """One WFA2 aligner (penalties, memory mode) whose span is set per pair."""

    def __init__(self, pen, memory_mode=0):
        self.r = oracle_lib.ref()
        self.lib = C.CDLL(oracle_lib.REF_SO)
        self.lib.wavefront_aligner_set_alignment_free_ends.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        self.lib.wavefront_aligner_set_alignment_free_ends.restype = None
        self.h = self.r.ref_new(pen[0], pen[1], pen[2], memory_mode, 0)
        self.wf = C.c_void_p.from_address(self.h).value      # (the handle's first field: the wavefront_aligner_t*)

    def align(self, p, t, span):
        pb, pe, tb, te = clamp_span(span, len(p), len(t))
        self.lib.wavefront_aligner_set_alignment_free_ends(self.wf, pb, pe, tb, te)
        cap = 2 * (len(p) + len(t)) + 16
        out = C.create_string_buffer(cap)
        s = self.r.ref_run(self.h, p, len(p), t, len(t), out, cap)
        return s, out.value.decode()

    def close(self):
        if self.h:
            self.r.ref_delete(self.h)
            self.h = None


def wfa2_endsfree(pairs, spans, pens, memory_mode=0):
    """-> (scores, cigars) of WFA2 for every (pattern, text), span, penalties."""
    aligners = {}
    scores, cigars = [], []
    try:
        for (p, t), span, pen in zip(pairs, spans, pens):
            al = aligners.get(tuple(pen))
            if al is None:
                al = aligners[tuple(pen)] = Wfa2EndsFree(pen, memory_mode)
            s, c = al.align(p, t, span)
            scores.append(s)
            cigars.append(c)
    finally:
        for al in aligners.values():
            al.close()
    return np.array(scores, dtype=np.int32), cigars


def dp_endsfree_score(p, t, pen, span):
    """Optimal ends-free gap-affine score (match 0, mismatch x, a gap of n bases o + n e), bytes compared as they are."""
    x, o, e = pen
    plen, tlen = len(p), len(t)
    pb, pe, tb, te = clamp_span(span, plen, tlen)
    INF = 1 << 40
    P = np.frombuffer(bytes(p), dtype=np.uint8)
    T = np.frombuffer(bytes(t), dtype=np.uint8)
    idx = np.arange(tlen + 1, dtype=np.int64)

    def with_insertions(base):
        # H[j] = min(base[j], min over j' < j of base[j'] + o + e (j - j')): a running minimum of base[j'] + o - e j'
        run = np.minimum.accumulate(base + o - e * idx)
        ins = np.full(tlen + 1, INF, dtype=np.int64)
        ins[1:] = run[:-1] + e * idx[1:]
        return np.minimum(base, ins)

    base = np.full(tlen + 1, INF, dtype=np.int64)
    base[:tb + 1] = 0                     # free starts on the first row
    H = with_insertions(base)
    D = np.full(tlen + 1, INF, dtype=np.int64)
    best = INF
    if plen <= pe:
        best = min(best, int(H[tlen]))   # the text is used up with the whole pattern left free (row 0)
    for i in range(1, plen + 1):
        D = np.minimum(H + o + e, D + e)
        base = D.copy()
        base[1:] = np.minimum(base[1:], H[:-1] + np.where(T == P[i - 1], 0, x))
        if i <= pb:
            base[0] = 0                   # free starts on the first column
        H = with_insertions(base)
        if plen - i <= pe:
            best = min(best, int(H[tlen]))
    # the pattern is used up with at most te text bases left
    best = min(best, int(H[tlen - te:].min()))
    return best


_ITEM = re.compile(r"(\d+)([MXID])")


def parse_cigar(cigar):
    items = [(int(n), op) for n, op in _ITEM.findall(cigar)]
    assert "".join(f"{n}{op}" for n, op in items) == cigar, f"malformed CIGAR {cigar!r}"
    return items


def check_cigar(p, t, cigar, pen, span, ends=None):
    """-> (valid, cost).  valid: the CIGAR is run-length encoded without equal neighbours, covers both whole sequences, M sits on equal
    and X on different bytes.  cost: its gap-affine cost WITHOUT the free bases: a leading D (I) run is free for as many bases as
    pattern_begin_free (text_begin_free) allows, a trailing one for pattern_end_free (text_end_free) -- or, with ends = (k0, k1),
    for exactly the bases those diagonals say (valid then also asks that the runs are there and the diagonals lie in the span)."""
    x, o, e = pen
    plen, tlen = len(p), len(t)
    pb, pe, tb, te = clamp_span(span, plen, tlen)
    items = parse_cigar(cigar)
    valid = all(n > 0 for n, _ in items) and all(a[1] != b[1] for a, b in zip(items, items[1:]))
    v = h = 0
    for n, op in items:
        if op in "MX":
            if v + n > plen or h + n > tlen:
                return False, -1
            eq = np.frombuffer(bytes(p[v:v + n]), dtype=np.uint8) == np.frombuffer(bytes(t[h:h + n]), dtype=np.uint8)
            valid &= bool(eq.all()) if op == "M" else bool((~eq).all())
            v += n
            h += n
        elif op == "I":
            h += n
        else:
            v += n
    valid &= v == plen and h == tlen
    free = [0] * len(items)
    if items:
        if ends is None:
            n, op = items[0]
            lead = min(n, tb if op == "I" else pb if op == "D" else 0)
            free[0] += lead
            n, op = items[-1]
            room = n - (lead if len(items) == 1 else 0)
            free[-1] += min(room, te if op == "I" else pe if op == "D" else 0)
        else:
            k0, k1 = int(ends[0]), int(ends[1])
            kend = tlen - plen
            valid &= -pb <= k0 <= tb and kend - te <= k1 <= kend + pe
            if k0:
                valid &= items[0][1] == ("I" if k0 > 0 else "D") and items[0][0] >= abs(k0)
                free[0] += abs(k0)
            if k1 != kend:
                valid &= items[-1][1] == ("D" if k1 > kend else "I")
                free[-1] += abs(k1 - kend)
                valid &= items[-1][0] >= free[-1]
    cost = 0
    for (n, op), f in zip(items, free):
        if op == "X":
            cost += x * n
        elif op in "ID" and n > f:
            cost += o + e * (n - f)
    return bool(valid), cost


# ---- the golden sets -----------------------------------------------------------------------------------------------------------
# The PAIRS of a set are not stored: make_set() rebuilds them, bit for bit on every machine, from a counter-based generator (splitmix64
# in numpy uint64 arithmetic: no library's random stream is relied on).  Stored are WFA2's answers, tests/golden/endsfree.<set>.alg,
# one "-score<TAB>CIGAR" line per pair like the other .alg fixtures ("*": an empty CIGAR); tests/golden/make_golden_endsfree.py writes them.
#   small      400 pairs of 0-300 bases (an empty pattern and an empty text among them): half of them a read inside a padded window, the
#              rest unrelated; thirteen hold N / IUPAC bytes.  Pair i runs under span kind i % 9 and penalties PENS[i % 4].
#   wide       8 pairs per start width pbf + tbf + 1 in {63, 64, 65, 129, 257, 1025} (the lane, wave and workgroup boundaries of the row
#              of score 0 and of the termination scan), 1.1-1.3 kbp at ~5 % error; the width split evenly, all on the pattern, all on
#              the text.
#   ties       32 pairs, text = the pattern repeated 3-5 times with sparse edits, both text ends free: several diagonals end the
#              alignment at the same score, the lowest must win.
#   small_t50  the pairs of `small`, ALL under the span (0,0,50,50) and penalties (2,3,1): a whole call under one span.
PENS = ((2, 3, 1), (5, 3, 2), (3, 1, 4), (4, 0, 2))
SMALL_SPANS = ((0, 0, 50, 50), (50, 0, 0, 50), (0, 50, 0, 50), (7, 13, 21, 9), (0, 0, 0, 30), (25, 0, 0, 0), (0, 0, INT_MAX, INT_MAX),
               (0, 0, 0, 0), (INT_MAX, INT_MAX, INT_MAX, INT_MAX))
WIDE_WIDTHS = (63, 64, 65, 129, 257, 1025)
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


class Rng:
    """splitmix64 over a counter."""

    def __init__(self, seed):
        self.seed, self.count = seed, 0

    def u64(self, n):
        z = np.arange(self.count + 1, self.count + 1 + n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z += np.full(1, self.seed, dtype=np.uint64) * np.uint64(0xD1342543DE82EF95)
        self.count += n
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))

    def integer(self, lo, hi):      # in [lo, hi)
        return lo + int(self.u64(1)[0] % np.uint64(hi - lo))

    def seq(self, n):
        return _ACGT[(self.u64(n) >> np.uint64(33)) % np.uint64(4)].tobytes()

    def mutate(self, s, rate):
        """Every base: deleted, a random base inserted in front of it, replaced by another base (a third of `rate` each), or kept."""
        n = len(s)
        r = (self.u64(n) >> np.uint64(11)).astype(np.float64) / float(1 << 53)
        extra = (self.u64(n) >> np.uint64(33)) % np.uint64(3)
        out = bytearray()
        for c, ri, x in zip(s, r, extra):
            if ri < rate / 3:
                continue
            if ri < 2 * rate / 3:
                out.append(b"ACGT"[int(x)])
                out.append(c)
            elif ri < rate:
                out.append(b"ACGT"[(b"ACGT".index(c) + 1 + int(x)) % 4])
            else:
                out.append(c)
        return bytes(out)


# ---- the pairs of the `sweep` sets (shared with affine2p_ref, wfadaptive_ref and linear_ref) --------------------------------------
# One parameter set of a sweep runs SWEEP_PAIRS short pairs; a budget equal to a pair's own score has to leave it on the one-wave tier,
# whose ring is (ring depth + I/D rows) rows of (window + 2 * ring depth + a chunk of padding) 16-bit cells in 40 KiB.  So a set with a
# deep ring (SWEEP_DEEP: depth >= 60, the ring alone is ~200 cells a row before the window) gets pairs of at most 48 bases and the others
# pairs of at most 160, and unrelated pairs -- the largest scores -- are half as long as the rest.
SWEEP_PAIRS, SWEEP_LONG, SWEEP_DEEP = 20, 5, 60


def ring_depth(pen):
    """Rows of the M ring the gap-affine kernels run under (x, o, e): one per score back to the deepest source, max(x, o + e) below, and
    the row being written -- of the penalties without their common factor, which the library divides out first."""
    return max(pen[0], pen[1] + pen[2]) // math.gcd(*pen) + 1


def sweep_top(depth):
    return 48 if depth >= SWEEP_DEEP else 160


def sweep_pairs(rng, top, which, unrelated=None):
    """SWEEP_PAIRS pairs of 0..top bases: 8 related at ~8 %, 4 unrelated, 4 with one planted gap of 1 to min(60, what fits) bases (the
    first one base, the second the longest; the side that carries the gap alternates), 2 repeats of unequal length (a homopolymer, a
    3-base tandem), 1 pair holding N (the byte-compare class), 1 pair with an empty side (the pattern where `which` is even)."""
    pairs = []
    for _ in range(8):
        p = rng.seq(rng.integer(top // 4, top + 1))
        pairs.append((p, rng.mutate(p, 0.08)[:top]))
    for _ in range(4):
        pairs.append((rng.seq(rng.integer(1, (unrelated or top // 2) + 1)), rng.seq(rng.integer(1, (unrelated or top // 2) + 1))))
    for j in range(4):
        base = rng.seq(rng.integer(3 * top // 8, 5 * top // 8 + 1))
        room = min(60, top - len(base))
        n = 1 if j == 0 else room if j == 1 else rng.integer(2, room)
        at = rng.integer(1, len(base))
        longer = base[:at] + rng.seq(n) + base[at:]
        pairs.append((base, longer) if j % 2 == 0 else (longer, base))
    for j in range(2):
        unit = rng.seq(1 if j == 0 else 3)
        left, right = rng.seq(rng.integer(4, top // 4)), rng.seq(rng.integer(4, top // 4))
        r1 = rng.integer(2, top // (4 * len(unit)))
        r2 = r1 + rng.integer(1, top // (8 * len(unit)) + 1)
        a, b = left + unit * r1 + right, left + unit * r2 + right
        pairs.append((a, b) if j == 0 else (b, a))
    p = rng.seq(rng.integer(top // 2, top + 1))
    t = rng.mutate(p, 0.08)[:top]
    pairs.append((p[:len(p) // 2] + b"N" + p[len(p) // 2 + 1:], t[:len(t) // 3] + b"N" + t[len(t) // 3 + 1:]))
    s = rng.seq(rng.integer(1, top // 4 + 1))
    pairs.append((b"", s) if which % 2 == 0 else (s, b""))
    assert len(pairs) == SWEEP_PAIRS
    return pairs


def sweep_long(rng):
    """SWEEP_LONG pairs of 600 to 700 bases (a few more with insertions) at ~4 %: 3 % substitutions and 1 % one-base indels, so that the score stays low enough for
    the one-wave tier under a deep ring while the rows (window and guard cells) run over several 64-lane chunks."""
    pairs = []
    for _ in range(SWEEP_LONG):
        p = rng.seq(rng.integer(600, 701))
        r = (rng.u64(len(p)) >> np.uint64(11)).astype(np.float64) / float(1 << 53)
        extra = (rng.u64(len(p)) >> np.uint64(33)) % np.uint64(3)
        out = bytearray()
        for c, ri, x in zip(p, r, extra):
            if ri < 0.005:
                continue
            if ri < 0.01:
                out.append(b"ACGT"[int(x)])
                out.append(c)
            elif ri < 0.04:
                out.append(b"ACGT"[(b"ACGT".index(c) + 1 + int(x)) % 4])
            else:
                out.append(c)
        pairs.append((p, bytes(out)))
    return pairs


def sweep_over(scores, budget, factor):
    """Pairs whose score lies above the budget the library runs under: the budget divided by the penalties' common factor, rounded down,
    and raised to 1 where that is 0 (8 under (9,9) is 1 under (1,1): a score of 9 is within it)."""
    return int((np.asarray(scores) > max(1, budget // factor) * factor).sum())


def sweep_budget_groups(keys, scores, factor, seed, limit=48):
    """The pairs of a sweep by (parameter key, golden score), for the runs under a budget of exactly that score and of one less:
    -> [(key, score, indices)], at most `limit` of them in a seeded order in which every key comes at least once.  Left out: score 0,
    and scores whose budget of one less is not below them once the library has divided it by the penalties' common factor (factor(key))
    and raised a budget under 1 to 1 -- (score - 1) // factor < 1: there the two budgets are the same run."""
    by = {}
    for i, (k, s) in enumerate(zip(keys, scores)):
        if int(s) > 0 and (int(s) - 1) // factor(k) >= 1:
            by.setdefault((k, int(s)), []).append(i)
    order = sorted(by)
    order = [order[j] for j in np.argsort(Rng(seed).u64(len(order)), kind="stable")]
    first = {}
    for ks in order:
        first.setdefault(ks[0], ks)
    assert len(first) <= limit
    chosen = list(first.values()) + [ks for ks in order if first[ks[0]] != ks]
    return [(k, s, by[(k, s)]) for k, s in chosen[:limit]]


#   sweep      SWEEP_PAIRS short pairs (sweep_pairs) per penalty set of SWEEP_PENS, pair i under SWEEP_SPANS[i % 5]; SWEEP_LONG long pairs
#              (sweep_long) under each of SWEEP_LONG_PENS -- M rings of 33 and 66 rows, either side of the one-wave tier's limit of 64 --, one per span.
#              Penalties: the cheapest; a coprime set; a common factor of 3; a mismatch deeper than 32; o + e = 64 with a common factor of 2
#              (the kernels run (1,31,1): an M ring of 33 rows); o + e = 65; e > x; o + e = 63: a ring of 64 rows, the deepest of the one-wave tier.
SWEEP_SET = "sweep"
SWEEP_PENS = ((1, 0, 1), (7, 2, 3), (6, 9, 3), (40, 2, 1), (2, 62, 2), (2, 63, 2), (3, 1, 6), (3, 61, 2))
SWEEP_LONG_PENS = ((2, 62, 2), (2, 63, 2))
SWEEP_SPANS = ((0, 0, 30, 30), (30, 30, 0, 0), (11, 0, 0, 17), (0, 0, 0, 0), (INT_MAX, INT_MAX, INT_MAX, INT_MAX))


def make_set(name):
    """-> (pairs, spans, pens) of a golden set."""
    pairs, spans, pens = [], [], []
    if name == SWEEP_SET:
        rng = Rng(20261001)
        for j, pen in enumerate(SWEEP_PENS):
            for i, pair in enumerate(sweep_pairs(rng, sweep_top(ring_depth(pen)), j)):
                pairs.append(pair)
                spans.append(SWEEP_SPANS[(i + j) % 5])
                pens.append(pen)
        for pen in SWEEP_LONG_PENS:
            for i, pair in enumerate(sweep_long(rng)):
                pairs.append(pair)
                spans.append(SWEEP_SPANS[i % 5])
                pens.append(pen)
    elif name in ("small", ONE_SPAN_SET):
        rng = Rng(20260101)
        for i in range(400):
            kind = i % 9
            if i == 9:
                p, t = b"", rng.seq(57)
            elif i == 18:
                p, t = rng.seq(41), b""
            elif i % 2 == 0:
                read = rng.seq(rng.integer(20, 200))
                lead, tail = rng.seq(rng.integer(0, 51)), rng.seq(rng.integer(0, 51))
                if kind in (1, 5):      # overlap shapes: the pattern sticks out in front
                    p, t = lead + read, rng.mutate(read, 0.06) + tail
                else:
                    p, t = read, lead + rng.mutate(read, 0.06) + tail
            else:
                p, t = rng.seq(rng.integer(1, 301)), rng.seq(rng.integer(1, 301))
            if i % 31 == 5 and len(p) > 4 and len(t) > 4:      # bytes outside ACGT: the byte-compare class
                p = p[:len(p) // 2] + b"N" + p[len(p) // 2 + 1:]
                t = t[:len(t) // 3] + b"NRY"[i % 3:i % 3 + 1] + t[len(t) // 3 + 1:]
            pairs.append((p, t))
            spans.append(SMALL_SPANS[kind] if name == "small" else ONE_SPAN)
            pens.append(PENS[i % 4] if name == "small" else ONE_SPAN_PEN)
    elif name == "wide":
        rng = Rng(20260102)
        for w in WIDE_WIDTHS:
            for j in range(8):
                pbf = ((w - 1) // 2, w - 1, 0)[j % 3]
                tbf = w - 1 - pbf
                core = rng.seq(rng.integer(1100, 1150))
                lead_p, lead_t = rng.seq(rng.integer(0, min(pbf, 100) + 1)), rng.seq(rng.integer(0, min(tbf, 100) + 1))
                pairs.append((lead_p + core, lead_t + rng.mutate(core, 0.05) + rng.seq(rng.integer(0, 20))))
                spans.append((pbf, 5, tbf, 30))
                pens.append((2, 3, 1))
    elif name == "ties":
        rng = Rng(20260103)
        for i in range(32):
            p = rng.seq(rng.integer(40, 81))
            pairs.append((p, rng.mutate(p * rng.integer(3, 6), 0.02 if i % 4 else 0.0)))
            spans.append((0, 0, 1000, 1000))
            pens.append((2, 3, 1))
    else:
        raise ValueError(name)
    return pairs, spans, pens


def golden_path(name):
    return os.path.join(GOLDEN, f"endsfree.{name}.alg")


def write_golden(name, scores, cigars):
    with open(golden_path(name), "w") as f:
        for s, c in zip(scores, cigars):
            f.write(f"{-int(s)}\t{c or '*'}\n")


def read_golden(name):
    """-> dict(pairs=[(pattern, text) bytes], spans=[4-tuples], pens=[3-tuples], scores=int32[n], cigars=[str])"""
    pairs, spans, pens = make_set(name)
    scores, cigars = [], []
    with open(golden_path(name)) as f:
        for line in f:
            s, c = line.rstrip("\n").split("\t")
            scores.append(-int(s))
            cigars.append("" if c == "*" else c)
    assert len(pairs) == len(scores)
    return dict(pairs=pairs, spans=spans, pens=pens, scores=np.array(scores, dtype=np.int32), cigars=cigars)


def groups(g):
    """Indices of a golden set by (span, penalties): one device call each."""
    out = {}
    for i, key in enumerate(zip(g["spans"], g["pens"])):
        out.setdefault(key, []).append(i)
    return out
