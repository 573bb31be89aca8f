"""Ground truth for the edit, indel and gap-linear distances (WFA2's one-component metrics) -- test infrastructure only.

  wfa2_linear        WFA2 itself, through the reference library that oracle/Makefile compiles in place (oracle/_ref/libwfa2ref.so,
                     optional): a copy of the exported wavefront_aligner_attr_default with the metric and linear_penalties written
                     into its leading int fields, then wavefront_aligner_new, wavefront_aligner_set_heuristic_none and ref_run()
  dp_linear_score    a plain dynamic program with one matrix (numpy, one vector step per row), independent of WFA2
  check_cigar_linear validity of a CIGAR and its cost under the metric; an X under indel is not valid
  wfa_linear_model   a plain restatement of the M-only wavefront search and its backtrace in numpy, without WFA2's exact pruning of
                     wide edit rows: slow and obvious, it shows on the CPU that "no pruning, mismatch > deletion > insertion" gives
                     WFA2's bytes
  make_set / read_golden   the golden sets: pairs rebuilt by a deterministic recipe, WFA2's answers in tests/golden/linear.<set>.alg

A metric is ("edit",), ("indel",) or ("linear", x, g): match 0, mismatch x > 0, every gap base g > 0; edit is (1, 1); indel is g = 1
without a mismatch move."""
import ctypes as C
import math
import os

import numpy as np

import oracle_lib
from affine2p_ref import _elf_symbol_size, _plant
from endsfree_ref import SWEEP_LONG, SWEEP_PAIRS, Rng, parse_cigar, sweep_long, sweep_pairs, sweep_top

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
EDIT, INDEL = ("edit",), ("indel",)
# edit; indel; WFA2's default with a common factor; a coprime pair; x < g; x > 2 g (a mismatch never beats an insertion plus a deletion)
METRICS = (EDIT, INDEL, ("linear", 4, 2), ("linear", 3, 2), ("linear", 1, 3), ("linear", 5, 1))
SETS = ("small", "small_edit", "ties", "lanes", "wide")
LONG_SET = "long"      # (kept out of SETS: the dynamic program and the model would take minutes on it)
WFA2_METRIC = {"indel": 0, "edit": 1, "linear": 2}      # distance_metric_t (wavefront_penalties.h)
GAP_AFFINE = 3
ATTR_METRIC_OFF, ATTR_LINEAR_OFF = 0, 28     # wavefront_aligner_attr_t: distance_metric; linear_penalties = {match, mismatch, indel}


# Cross-check against the emulation a caller had before these metrics (gap-affine with a zero opening): on tests/golden/seq1k.seq WFA2
# gap-linear (x, g) and WFA2 gap-affine (x, 0, g) -- and edit against (1, 0, 1) -- give the same scores AND the same CIGAR bytes.  Found
# with WFA2 run live and asserted again by tests/test_linear_cpu.py wherever oracle/_ref exists; the GPU cross-check compares CIGAR
# bytes because of it.
SEQ1K_CROSS = ((("linear", 3, 2), (3, 0, 2)), (("linear", 4, 2), (4, 0, 2)), (("linear", 5, 1), (5, 0, 1)), (EDIT, (1, 0, 1)))
SEQ1K_CIGARS_AGREE = True


def pens_of(metric):
    """-> (x, g); x is None under indel."""
    if metric[0] == "edit":
        return 1, 1
    if metric[0] == "indel":
        return None, 1
    return int(metric[1]), int(metric[2])


class Wfa2Linear:
    """One WFA2 aligner under an edit, indel or gap-linear metric."""

    def __init__(self, metric):
        self.r = oracle_lib.ref()
        self.lib = C.CDLL(oracle_lib.REF_SO)
        size = _elf_symbol_size(oracle_lib.REF_SO, "wavefront_aligner_attr_default")
        attr = (C.c_char * size).from_buffer_copy((C.c_char * size).in_dll(self.lib, "wavefront_aligner_attr_default"))
        ints = C.cast(attr, C.POINTER(C.c_int))
        assert ints[ATTR_METRIC_OFF // 4] == GAP_AFFINE, "the default attributes start with distance_metric = gap_affine"
        assert tuple(ints[ATTR_LINEAR_OFF // 4 + i] for i in range(3)) == (0, 4, 2), "linear_penalties at bytes 28-39"
        ints[ATTR_METRIC_OFF // 4] = WFA2_METRIC[metric[0]]
        if metric[0] == "linear":
            for i, v in enumerate((0, metric[1], metric[2])):
                ints[ATTR_LINEAR_OFF // 4 + i] = int(v)
        self.lib.wavefront_aligner_new.argtypes = [C.c_void_p]
        self.lib.wavefront_aligner_new.restype = C.c_void_p
        self.lib.wavefront_aligner_set_heuristic_none.argtypes = [C.c_void_p]
        self.lib.wavefront_aligner_set_heuristic_none.restype = None
        self.lib.wavefront_aligner_delete.argtypes = [C.c_void_p]
        self.lib.wavefront_aligner_delete.restype = None
        self.wf = self.lib.wavefront_aligner_new(C.addressof(attr))
        self.lib.wavefront_aligner_set_heuristic_none(self.wf)
        self.handle = C.c_void_p(self.wf)      # (what ref_run takes: a struct whose first field is the wavefront_aligner_t*)

    def align(self, p, t):
        cap = 2 * (len(p) + len(t)) + 16
        out = C.create_string_buffer(cap)
        s = self.r.ref_run(C.addressof(self.handle), p, len(p), t, len(t), out, cap)
        # (ref_run negates cigar->score and WFA2's sign differs by metric: the magnitude is checked against the dynamic program)
        return abs(s), out.value.decode()

    def close(self):
        if self.wf:
            self.lib.wavefront_aligner_delete(self.wf)
            self.wf = None


def wfa2_linear(pairs, metrics):
    """-> (scores, cigars) of WFA2 for every (pattern, text) under its metric."""
    aligners = {}
    scores, cigars = [], []
    try:
        for (p, t), m in zip(pairs, metrics):
            al = aligners.get(tuple(m))
            if al is None:
                al = aligners[tuple(m)] = Wfa2Linear(m)
            s, c = al.align(p, t)
            scores.append(s)
            cigars.append(c)
    finally:
        for al in aligners.values():
            al.close()
    return np.array(scores, dtype=np.int32), cigars


def dp_linear_score(p, t, x, g):
    """Optimal end-to-end score: match 0, mismatch x (None: no mismatch move, indel), every gap base g; bytes compared as they are.
    One matrix, a row at a time: vertical and diagonal moves in one vector step, horizontal ones as a running minimum."""
    plen, tlen = len(p), len(t)
    INF = 1 << 40
    P = np.frombuffer(bytes(p), dtype=np.uint8)
    T = np.frombuffer(bytes(t), dtype=np.uint8)
    idx = np.arange(tlen + 1, dtype=np.int64)
    H = g * idx
    for i in range(1, plen + 1):
        base = H + g
        base[1:] = np.minimum(base[1:], H[:-1] + np.where(T == P[i - 1], 0, INF if x is None else x))
        H = np.minimum.accumulate(base - g * idx) + g * idx
    return int(H[tlen])


def check_cigar_linear(p, t, cigar, metric):
    """-> (valid, cost).  valid: the CIGAR is run-length encoded without equal neighbours, covers both whole sequences, M sits on equal
    and X on different bytes, and there is no X under indel.  cost: x per mismatch, g per gap base."""
    x, g = pens_of(metric)
    plen, tlen = len(p), len(t)
    items = parse_cigar(cigar)
    valid = all(n > 0 for n, _ in items) and all(a[1] != b[1] for a, b in zip(items, items[1:]))
    v = h = cost = 0
    for n, op in items:
        if op in "MX":
            if v + n > plen or h + n > tlen:
                return False, -1
            eq = np.frombuffer(bytes(p[v:v + n]), dtype=np.uint8) == np.frombuffer(bytes(t[h:h + n]), dtype=np.uint8)
            valid &= bool(eq.all()) if op == "M" else bool((~eq).all())
            v += n
            h += n
            if op == "X":
                valid &= x is not None
                cost += (x or 0) * n
        else:
            if op == "I":
                h += n
            else:
                v += n
            cost += g * n
    valid &= v == plen and h == tlen
    return bool(valid), cost


# ---- the model -------------------------------------------------------------------------------------------------------------------
NULL = -(1 << 30)


def wfa_linear_model(p, t, metric):
    """-> (score, cigar): the M-only wavefront search as WFA2 runs it (wavefront_compute_linear.c, wavefront_compute_edit.c: recurrence,
    nulling, extension, limits from the trimmed input rows, end trimming) WITHOUT the exact pruning of wide edit rows, and WFA2's
    backtrace (wavefront_backtrace.c:223-317: on equal offsets mismatch, then deletion, then insertion)."""
    x, g = pens_of(metric)
    plen, tlen = len(p), len(t)
    kend = tlen - plen
    P = np.frombuffer(bytes(p) + b"\0", dtype=np.uint8)
    T = np.frombuffer(bytes(t) + b"\0", dtype=np.uint8)

    def extend(ks, offs):
        h = offs.copy()
        v = h - ks
        act = np.nonzero((h >= 0) & (v < plen) & (h < tlen))[0]
        while act.size:
            act = act[P[v[act]] == T[h[act]]]
            h[act] += 1
            v[act] += 1
            act = act[(v[act] < plen) & (h[act] < tlen)]
        return h

    def read(row, ks):      # offsets of a row on diagonals ks; NULL outside its limits, or where there is no row
        out = np.full(ks.shape, NULL, dtype=np.int64)
        if row is not None:
            lo, hi, arr = row
            m = (ks >= lo) & (ks <= hi)
            out[m] = arr[ks[m] - lo]
        return out

    rows = [(0, 0, extend(np.array([0]), np.array([0], dtype=np.int64)))]
    s = 0
    while True:
        row = rows[s]
        if row is not None and row[0] <= kend <= row[1] and row[2][kend - row[0]] >= tlen:
            break
        s += 1
        assert s <= 2 * g * min(plen, tlen) + g * abs(kend), "no alignment costs more"
        in_x = rows[s - x] if x is not None and s >= x else None
        in_g = rows[s - g] if s >= g else None
        if in_x is None and in_g is None:
            rows.append(None)
            continue
        # (a missing row carries lo = 1, hi = -1: wavefront_compute.c:41-60)
        lx, hx = (in_x[0], in_x[1]) if in_x is not None else (1, -1)
        lg, hg = (in_g[0], in_g[1]) if in_g is not None else (1, -1)
        lo, hi = (min(lx, lg - 1), max(hx, hg + 1)) if x is not None else (lg - 1, hg + 1)
        ks = np.arange(lo, hi + 1)
        best = np.maximum(read(in_g, ks - 1) + 1, read(in_g, ks + 1))
        if x is not None:
            best = np.maximum(best, read(in_x, ks) + 1)
        ok = (best >= 0) & (best <= tlen) & (best - ks >= 0) & (best - ks <= plen)
        arr = extend(ks, np.where(ok, best, NULL))
        good = np.nonzero(arr >= 0)[0]      # end trimming (wavefront_compute.c:570-603)
        rows.append(None if good.size == 0 else (lo + int(good[0]), lo + int(good[-1]), arr[good[0]:good[-1] + 1]))

    def at(sc, k, add):      # (offset + add, or NULL) of M[sc][k]
        if sc < 0 or rows[sc] is None or not rows[sc][0] <= k <= rows[sc][1]:
            return NULL
        o = int(rows[sc][2][k - rows[sc][0]])
        return o + add if o >= 0 else NULL

    ops = []      # reversed
    score, k, off = s, kend, tlen
    v, h = off - k, off
    while v > 0 and h > 0 and score > 0:
        # (type ranks of wavefront_backtrace.c:49-59: M 9, D1_open 5, I1_open 1)
        cands = [(at(score - x, k, 1), 9, "X") if x is not None else (NULL, 9, "X"), (at(score - g, k + 1, 0), 5, "D"), (at(score - g, k - 1, 1), 1, "I")]
        src, _, op = max(cands)
        if src < 0:
            break
        ops.append(("M", off - src))
        off = src
        v, h = off - k, off
        if v <= 0 or h <= 0:
            break
        ops.append((op, 1))
        if op == "X":
            score -= x
            off -= 1
        elif op == "I":
            score -= g
            k -= 1
            off -= 1
        else:
            score -= g
            k += 1
        v, h = off - k, off
    if v > 0 and h > 0:
        n = min(v, h)
        ops.append(("M", n))
        v -= n
        h -= n
    ops.append(("D", v))
    ops.append(("I", h))
    out, run, cur = [], 0, None
    for op, n in reversed(ops):
        if n == 0:
            continue
        if op != cur:
            if cur is not None:
                out.append(f"{run}{cur}")
            cur, run = op, 0
        run += n
    if cur is not None:
        out.append(f"{run}{cur}")
    return s, "".join(out)


# ---- the golden sets -----------------------------------------------------------------------------------------------------------
# The PAIRS of a set are not stored: make_set() rebuilds them, bit for bit on every machine, from the counter-based generator of
# endsfree_ref (Rng).  Stored are WFA2's answers, tests/golden/linear.<set>.alg, one "-score<TAB>CIGAR" line per pair like the other
# .alg fixtures ("*": an empty CIGAR); tests/golden/make_golden_linear.py writes them.
#   small       the 400-pair recipe of affine2p_ref's `small`: 0-300 bases, half related at ~6 %, half unrelated; an empty pattern, an
#               empty text and an identical pair; thirteen hold N / IUPAC bytes.  Pair i runs under METRICS[i % 6].
#   small_edit  the same pairs, all under edit: a whole call, command line or seam batch.
#   ties        32 pairs with a homopolymer run or a 2-6 base tandem repeat from which a few bases are cut or into which they are put,
#               plus 0-1 % noise: the gap can sit anywhere in the repeat, the priority decides the bytes.  Edit, indel, linear(3,2) by turns.
#   lanes       24 pairs of 1.1-1.3 kbp at ~3 % noise with one to three planted indels of 63, 64, 65 or 200 bases: rows cross lane and
#               wave boundaries.  Edit, indel, linear(4,2), linear(5,1) by turns.
#   wide        4 pairs whose edit rows pass 1000 diagonals (WFA2's exact pruning is active): 600 against 3000 unrelated bases and the
#               reverse, 2500 against 2600, 1500 against 1500.  Edit; the first two once more under indel.
#   long        2 pairs of 33.5 kbp at ~0.5 % noise with a planted indel of 300 bases, under edit: the tier with 32-bit offsets.
TIES_METRICS = (EDIT, INDEL, ("linear", 3, 2))
LANES_METRICS = (EDIT, INDEL, ("linear", 4, 2), ("linear", 5, 1))
GAP_LENGTHS = (63, 64, 65, 200)
#   sweep       SWEEP_PAIRS short pairs (endsfree_ref.sweep_pairs) under each of SWEEP_METRICS; SWEEP_LONG long pairs (sweep_long) under
#               each of SWEEP_LONG_METRICS, M rings of 64 and 65 rows: either side of the one-wave tier's limit.
SWEEP_SET = "sweep"
# edit as gap-linear; x > g and x < g, coprime; two sets with a common factor (3 and 9); a mismatch deeper than 32, without and with a
# deeper gap base; rings of 64, 65 and 66 rows by the mismatch, then by the gap base; a gap base deeper than 32.  WFA2 accepts all fifteen.
SWEEP_METRICS = tuple(("linear", x, g) for x, g in ((1, 1), (2, 1), (7, 2), (2, 7), (6, 3), (9, 9), (33, 1), (40, 3), (63, 1), (64, 1), (65, 1),
                                                    (1, 63), (1, 64), (1, 65), (3, 40)))
SWEEP_LONG_METRICS = (("linear", 63, 1), ("linear", 64, 1))


def ring_depth(metric):
    """Rows of the M ring the kernels run: one per score back to the deepest source, max(x, g) below, and the row being written -- of
    the penalties without their common factor, which the library divides out first."""
    x, g = pens_of(metric)
    return max(x or 0, g) // math.gcd(x or g, g) + 1


def make_set(name):
    """-> (pairs, metrics) of a golden set."""
    pairs, metrics = [], []
    if name == SWEEP_SET:
        rng = Rng(20261003)
        for j, m in enumerate(SWEEP_METRICS):
            pairs += sweep_pairs(rng, sweep_top(ring_depth(m)), j)
            metrics += [m] * SWEEP_PAIRS
        for m in SWEEP_LONG_METRICS:
            pairs += sweep_long(rng)
            metrics += [m] * SWEEP_LONG
    elif name in ("small", "small_edit"):
        rng = Rng(20260201)
        for i in range(400):
            if i == 9:
                p, t = b"", rng.seq(57)
            elif i == 18:
                p, t = rng.seq(41), b""
            elif i == 27:
                p = rng.seq(133)
                t = p
            elif i % 2 == 0:
                p = rng.seq(rng.integer(20, 301))
                t = rng.mutate(p, 0.06)[:300]
            else:
                p, t = rng.seq(rng.integer(1, 301)), rng.seq(rng.integer(1, 301))
            if i % 31 == 5 and len(p) > 4 and len(t) > 4:      # bytes outside ACGT: the byte-compare class
                p = p[:len(p) // 2] + b"N" + p[len(p) // 2 + 1:]
                t = t[:len(t) // 3] + b"NRY"[i % 3:i % 3 + 1] + t[len(t) // 3 + 1:]
            pairs.append((p, t))
            metrics.append(METRICS[i % 6] if name == "small" else EDIT)
    elif name == "ties":
        rng = Rng(20260301)
        for i in range(32):
            cut = rng.integer(1, 7)
            unit = rng.seq(1 if i % 4 < 2 else rng.integer(2, 7))
            reps = (cut + len(unit) - 1) // len(unit) * 2 + rng.integer(2, 6)
            left, right = rng.seq(rng.integer(60, 140)), rng.seq(rng.integer(60, 140))
            long_run, short_run = unit * reps, (unit * reps)[cut:]
            a, b = left + long_run + right, left + short_run + right
            p, t = (a, b) if i % 8 < 4 else (b, a)
            pairs.append((p, rng.mutate(t, 0.01 if i % 3 == 0 else 0.0)))
            metrics.append(TIES_METRICS[i % 3])
    elif name == "lanes":
        rng = Rng(20260302)
        for i in range(24):
            planted, net = [], 0
            for j in range(1 + i % 3):
                n = GAP_LENGTHS[(i // 4 + 2 * j + i) % len(GAP_LENGTHS)]
                insert = (i // 4 + i) % 2 == 0 if j == 0 else net < 0
                planted.append((n, insert))
                net += n if insert else -n
            p = rng.seq(1200 - net // 2 + rng.integer(-10, 11))
            t = rng.mutate(p, 0.03)
            for n, insert in planted:
                t = _plant(rng, t, n, insert)
            pairs.append((p, t))
            metrics.append(LANES_METRICS[i % 4])
    elif name == "wide":
        rng = Rng(20260303)
        four = [(rng.seq(600), rng.seq(3000)), (rng.seq(3000), rng.seq(600)), (rng.seq(2500), rng.seq(2600)), (rng.seq(1500), rng.seq(1500))]
        pairs = four + four[:2]
        metrics = [EDIT] * 4 + [INDEL] * 2
    elif name == LONG_SET:
        rng = Rng(20260305)
        for i in range(2):
            p = rng.seq(33500 + 37 * i)
            pairs.append((p, _plant(rng, rng.mutate(p, 0.005), 300, insert=i == 0)))
            metrics.append(EDIT)
    else:
        raise ValueError(name)
    return pairs, metrics


def golden_path(name):
    return os.path.join(GOLDEN, f"linear.{name}.alg")


def write_golden(name, scores, cigars):
    with open(golden_path(name), "w") as f:
        for s, c in zip(scores, cigars):
            f.write(f"{-int(s)}\t{c or '*'}\n")


_golden_cache = {}


def read_golden(name):
    """-> dict(pairs=[(pattern, text) bytes], metrics=[tuples], scores=int32[n], cigars=[str]); read once, shared, not to be changed"""
    if name in _golden_cache:
        return _golden_cache[name]
    pairs, metrics = make_set(name)
    scores, cigars = [], []
    with open(golden_path(name)) as f:
        for line in f:
            s, c = line.rstrip("\n").split("\t")
            scores.append(-int(s))
            cigars.append("" if c == "*" else c)
    assert len(pairs) == len(scores)
    _golden_cache[name] = dict(pairs=pairs, metrics=metrics, scores=np.array(scores, dtype=np.int32), cigars=cigars)
    return _golden_cache[name]


def groups(g):
    """Indices of a golden set by metric: one device call each."""
    out = {}
    for i, m in enumerate(g["metrics"]):
        out.setdefault(tuple(m), []).append(i)
    return out
