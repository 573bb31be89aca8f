"""Ground truth for the edit, indel and gap-linear distances under an ends-free span ("infix" edit distance) -- test infrastructure only.

  wfa2_linear_endsfree       WFA2 itself: a linear_ref.Wfa2Linear per metric with wavefront_aligner_set_alignment_free_ends called with
                             the clamped span before EVERY pair, zeros included (an aligner switched back and forth between end-to-end
                             and ends-free crashed inside WFA2 on an empty pattern; one that is always ends-free runs clean)
  dp_linear_endsfree_score   linear_ref.dp_linear_score with the free borders of endsfree_ref.dp_endsfree_score
  check_cigar_linear_span    endsfree_ref.check_cigar under a metric, its ends=(k0, k1) form included; an X under indel is not valid
  wfa_linear_endsfree_model  linear_ref.wfa_linear_model with the start row, the lowest-diagonal termination and the free runs: slow and
                             obvious, what to debug a kernel against
  make_set / read_golden     the golden sets: pairs rebuilt from the recipes of linear_ref and endsfree_ref, WFA2's answers in
                             tests/golden/linef.<set>.alg (tests/golden/make_golden_linear_endsfree.py writes them)

A metric is linear_ref's, a span endsfree_ref's."""
import ctypes as C
import os

import numpy as np

import endsfree_ref
import linear_ref
from affine2p_ref import _plant
from endsfree_ref import INT_MAX, SWEEP_SPANS, Rng, clamp_span, parse_cigar
from linear_ref import EDIT, LANES_METRICS, METRICS, NULL, TIES_METRICS, Wfa2Linear, pens_of

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
SETS = ("small", "small_edit_t50", "wide", "ties")
SWEEP_SET, LONG_SET = "sweep", "long"
ONE_SPAN = (0, 0, 50, 50)
LONG_SPAN = (0, 0, 200, 200)

# Against the emulation a caller had before (gap-affine (1, 0, 1) under the same span on the gap-affine ends-free kernels): on
# small_edit_t50 WFA2's scores agree on all 400 pairs; whether its CIGAR bytes do is a found fact, not an assumption -- found with WFA2
# run live (make_golden_linear_endsfree.py prints it) and asserted again by tests/test_linear_endsfree_cpu.py wherever oracle/_ref exists.
EMULATION_PEN = (1, 0, 1)
SMALL_EDIT_T50_CIGARS_AGREE = True


class Wfa2LinearEndsFree(Wfa2Linear):
    def __init__(self, metric):
        super().__init__(metric)
        self.lib.wavefront_aligner_set_alignment_free_ends.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        self.lib.wavefront_aligner_set_alignment_free_ends.restype = None

    def align_span(self, p, t, span):
        pb, pe, tb, te = clamp_span(span, len(p), len(t))
        self.lib.wavefront_aligner_set_alignment_free_ends(self.wf, pb, pe, tb, te)
        return self.align(p, t)


def wfa2_linear_endsfree(pairs, metrics, spans):
    """-> (scores, cigars) of WFA2 for every (pattern, text) under its metric and span."""
    aligners = {}
    scores, cigars = [], []
    try:
        for (p, t), m, span in zip(pairs, metrics, spans):
            al = aligners.get(tuple(m))
            if al is None:
                al = aligners[tuple(m)] = Wfa2LinearEndsFree(m)
            s, c = al.align_span(p, t, span)
            scores.append(s)
            cigars.append(c)
    finally:
        for al in aligners.values():
            al.close()
    return np.array(scores, dtype=np.int32), cigars


def dp_linear_endsfree_score(p, t, x, g, span):
    """Optimal ends-free score: match 0, mismatch x (None: indel), every gap base g; one matrix with free borders."""
    plen, tlen = len(p), len(t)
    pb, pe, tb, te = clamp_span(span, plen, tlen)
    INF = 1 << 40
    P = np.frombuffer(bytes(p), dtype=np.uint8)
    T = np.frombuffer(bytes(t), dtype=np.uint8)
    idx = np.arange(tlen + 1, dtype=np.int64)

    def with_insertions(base):
        return np.minimum.accumulate(base - g * idx) + g * idx

    base = np.full(tlen + 1, INF, dtype=np.int64)
    base[:tb + 1] = 0                     # free starts on the first row
    H = with_insertions(base)
    best = INF
    if plen <= pe:
        best = min(best, int(H[tlen]))   # the text is used up with the whole pattern left free (row 0)
    for i in range(1, plen + 1):
        base = H + g
        base[1:] = np.minimum(base[1:], H[:-1] + np.where(T == P[i - 1], 0, INF if x is None else x))
        if i <= pb:
            base[0] = 0                   # free starts on the first column
        H = with_insertions(base)
        if plen - i <= pe:
            best = min(best, int(H[tlen]))
    return min(best, int(H[tlen - te:].min()))      # the pattern is used up with at most te text bases left


def check_cigar_linear_span(p, t, cigar, metric, span, ends=None):
    """-> (valid, cost): endsfree_ref.check_cigar under (x, 0, g) -- validity, the free runs at the ends (or exactly those that
    ends = (k0, k1) say), cost without them -- and no X under indel."""
    x, g = pens_of(metric)
    valid, cost = endsfree_ref.check_cigar(p, t, cigar, (x if x is not None else 0, 0, g), span, ends=ends)
    if x is None and any(op == "X" for _, op in parse_cigar(cigar)):
        valid = False
    return valid, cost


def wfa_linear_endsfree_model(p, t, metric, span):
    """-> (score, cigar, (k0, k1)): linear_ref.wfa_linear_model with a start row on [-pbf, tbf] at offsets max(k, 0)
    (wavefront_unialign.c:137-178), the termination of wavefront_extend.c:124-170 -- the lowest diagonal of the extended row whose cell
    has used up the text with at most pef pattern bases left, or the pattern with at most tef text bases left -- and the free runs."""
    x, g = pens_of(metric)
    plen, tlen = len(p), len(t)
    kend = tlen - plen
    pb, pe, tb, te = clamp_span(span, plen, tlen)
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

    def read(row, ks):
        out = np.full(ks.shape, NULL, dtype=np.int64)
        if row is not None:
            lo, hi, arr = row
            m = (ks >= lo) & (ks <= hi)
            out[m] = arr[ks[m] - lo]
        return out

    def end_of(row):      # the lowest diagonal that ends the alignment, or None
        if row is None:
            return None
        lo, _, arr = row
        ks = np.arange(lo, lo + arr.size)
        v = arr - ks
        hit = (arr >= 0) & (((arr >= tlen) & (plen - v <= pe)) | ((v >= plen) & (tlen - arr <= te)))
        good = np.nonzero(hit)[0]
        return lo + int(good[0]) if good.size else None

    ks0 = np.arange(-pb, tb + 1)
    rows = [(-pb, tb, extend(ks0, np.maximum(ks0, 0).astype(np.int64)))]
    s = 0
    while True:
        k1 = end_of(rows[s])
        if k1 is not None:
            break
        s += 1
        assert s <= 2 * g * min(plen, tlen) + g * abs(kend), "no alignment costs more"
        in_x = rows[s - x] if x is not None and s >= x else None
        in_g = rows[s - g] if s >= g else None
        if in_x is None and in_g is None:
            rows.append(None)
            continue
        lx, hx = (in_x[0], in_x[1]) if in_x is not None else (1, -1)
        lg, hg = (in_g[0], in_g[1]) if in_g is not None else (1, -1)
        lo, hi = (min(lx, lg - 1), max(hx, hg + 1)) if x is not None else (lg - 1, hg + 1)
        ks = np.arange(lo, hi + 1)
        best = np.maximum(read(in_g, ks - 1) + 1, read(in_g, ks + 1))
        if x is not None:
            best = np.maximum(best, read(in_x, ks) + 1)
        ok = (best >= 0) & (best <= tlen) & (best - ks >= 0) & (best - ks <= plen)
        arr = extend(ks, np.where(ok, best, NULL))
        good = np.nonzero(arr >= 0)[0]
        rows.append(None if good.size == 0 else (lo + int(good[0]), lo + int(good[-1]), arr[good[0]:good[-1] + 1]))

    def at(sc, k, add):
        if sc < 0 or rows[sc] is None or not rows[sc][0] <= k <= rows[sc][1]:
            return NULL
        o = int(rows[sc][2][k - rows[sc][0]])
        return o + add if o >= 0 else NULL

    ops = []      # reversed
    score, k = s, k1
    off = int(rows[s][2][k1 - rows[s][0]])
    v, h = off - k, off
    ops.append(("I", tlen - h))      # what is left behind the end: free
    ops.append(("D", plen - v))
    while v > 0 and h > 0 and score > 0:
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
    k0 = h - v      # (the border cell the path starts from; beyond the free bases the gap along the border is paid)
    k0 = max(-pb, min(tb, k0))
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
    return s, "".join(out), (k0, k1)


# ---- the golden sets -----------------------------------------------------------------------------------------------------------
#   small           the 400 pairs and spans of endsfree_ref's `small`; pair i under METRICS[(i // 9) % 6]: the span kind is i % 9, so all
#                   54 span-kind by metric combinations occur
#   small_edit_t50  the pairs of endsfree_ref's `small_t50`, ALL under edit and the span (0,0,50,50): a whole call, seam batch or command line
#   wide            endsfree_ref's `wide` (start rows of 63, 64, 65, 129, 257, 1025 cells); pair i under LANES_METRICS[i % 4]
#   ties            endsfree_ref's `ties` (several end diagonals at one score); pair i under TIES_METRICS[i % 3]
#   sweep           the pairs and metrics of linear_ref's `sweep`; pair i of metric j under SWEEP_SPANS[(i + j) % 5], long pair i under [i % 5]
#   long            2 patterns of 33.5 kbp; text = 150 random bases + the pattern at ~0.5 % noise with a planted 300-base indel + 120 random
#                   bases; span (0,0,200,200), edit: the tier with 32-bit offsets
def make_set(name):
    """-> (pairs, metrics, spans) of a golden set."""
    if name == "small":
        pairs, spans, _ = endsfree_ref.make_set("small")
        return pairs, [METRICS[(i // 9) % 6] for i in range(len(pairs))], spans
    if name == "small_edit_t50":
        pairs, _, _ = endsfree_ref.make_set(endsfree_ref.ONE_SPAN_SET)
        return pairs, [EDIT] * len(pairs), [ONE_SPAN] * len(pairs)
    if name == "wide":
        pairs, spans, _ = endsfree_ref.make_set("wide")
        return pairs, [LANES_METRICS[i % 4] for i in range(len(pairs))], spans
    if name == "ties":
        pairs, spans, _ = endsfree_ref.make_set("ties")
        return pairs, [TIES_METRICS[i % 3] for i in range(len(pairs))], spans
    if name == SWEEP_SET:
        pairs, metrics = linear_ref.make_set(linear_ref.SWEEP_SET)
        spans = []
        n_short = len(linear_ref.SWEEP_METRICS) * endsfree_ref.SWEEP_PAIRS
        for j in range(len(linear_ref.SWEEP_METRICS)):
            spans += [SWEEP_SPANS[(i + j) % 5] for i in range(endsfree_ref.SWEEP_PAIRS)]
        for _ in linear_ref.SWEEP_LONG_METRICS:
            spans += [SWEEP_SPANS[i % 5] for i in range(endsfree_ref.SWEEP_LONG)]
        assert len(spans) == len(pairs) and n_short <= len(pairs)
        return pairs, metrics, spans
    if name == LONG_SET:
        rng = Rng(20261101)
        pairs = []
        for i in range(2):
            p = rng.seq(33500 + 37 * i)
            lead = rng.seq(150)
            core = _plant(rng, rng.mutate(p, 0.005), 300, insert=i == 0)
            pairs.append((p, lead + core + rng.seq(120)))
        return pairs, [EDIT] * 2, [LONG_SPAN] * 2
    raise ValueError(name)


def golden_path(name):
    return os.path.join(GOLDEN, f"linef.{name}.alg")


def write_golden(name, scores, cigars):
    with open(golden_path(name), "w") as f:
        for s, c in zip(scores, cigars):
            f.write(f"{-int(s)}\t{c or '*'}\n")


_golden_cache = {}


def read_golden(name):
    """-> dict(pairs, metrics, spans, scores=int32[n], cigars=[str]); read once, shared, not to be changed"""
    if name in _golden_cache:
        return _golden_cache[name]
    pairs, metrics, spans = make_set(name)
    scores, cigars = [], []
    with open(golden_path(name)) as f:
        for line in f:
            s, c = line.rstrip("\n").split("\t")
            scores.append(-int(s))
            cigars.append("" if c == "*" else c)
    assert len(pairs) == len(scores)
    _golden_cache[name] = dict(pairs=pairs, metrics=metrics, spans=spans, scores=np.array(scores, dtype=np.int32), cigars=cigars)
    return _golden_cache[name]


def groups(g):
    """Indices of a golden set by (metric, span): one device call each."""
    out = {}
    for i, key in enumerate(zip(map(tuple, g["metrics"]), map(tuple, g["spans"]))):
        out.setdefault(key, []).append(i)
    return out
