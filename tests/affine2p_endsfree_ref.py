"""Ground truth for two-piece gap-affine alignment under an ends-free span -- test infrastructure only, built on affine2p_ref and
endsfree_ref.

  wfa2_affine2p_endsfree     WFA2 itself: affine2p_ref.Wfa2Affine2p with wavefront_aligner_set_alignment_free_ends on its aligner
  dp_affine2p_endsfree_score the five-matrix numpy program of affine2p_ref with the free borders of endsfree_ref.dp_endsfree_score
  check_cigar2p_span         validity of a CIGAR and its cost without the free runs, every paid run priced min(o1 + n e1, o2 + n e2)
  make_set / read_golden     the golden sets; WFA2's answers in tests/golden/affine2p_ef.<set>.alg (written by running this module)

Sets (pairs rebuilt from endsfree_ref.Rng; penalties from affine2p_ref.PENS, spans from endsfree_ref.SMALL_SPANS):
  small      the first 200 pairs of endsfree_ref's `small` (reads in padded windows, overlap shapes, unrelated pairs, an empty pattern,
             an empty text, N / IUPAC bytes); pair i under PENS[i % 6] and SMALL_SPANS[i % 9]
  small_t50  the same pairs, all under (4,6,2,24,1) and (0,0,50,50)
  wide       3 pairs per start-row width pbf + tbf + 1 in WIDE_WIDTHS (split evenly, all on the pattern, all on the text), ~1.1 kbp at 3 %
  gaps       36 pairs of a ~600-base read with one planted indel of n* - 1, n* or n* + 1 bases under the two PENS with a whole crossover
             n*: mid-read, or flush against a free begin / end beyond the GAPS_FREE free bases -- the free and the paid run merge
  ties       16 pairs, text = the pattern repeated 3-5 times, both text ends free: the lowest of several end diagonals wins
  long       one pair of 33.5 kbp at 0.5 % with a 300-base indel inside a window: the 32-bit tier"""
import ctypes as C
import gzip
import os

import numpy as np

import affine2p_ref as a2
import endsfree_ref as ef
from endsfree_ref import Rng, clamp_span, parse_cigar

SETS = ("small", "wide", "gaps", "ties")
ONE_SET, ONE_PEN, ONE_SPAN = "small_t50", a2.DEFAULT_PEN, (0, 0, 50, 50)
LONG_SET = "long"      # (kept out of SETS: the dynamic program would take minutes on it)
WIDE_WIDTHS = (63, 64, 65, 129, 257)
GAPS_PENS = tuple(pen for pen in a2.PENS if a2.crossover(pen))
GAPS_FREE = 20


class Wfa2Affine2pEndsFree(a2.Wfa2Affine2p):
    def align(self, p, t, span):
        self.lib.wavefront_aligner_set_alignment_free_ends.argtypes = [C.c_void_p] + [C.c_int] * 4
        self.lib.wavefront_aligner_set_alignment_free_ends.restype = None
        self.lib.wavefront_aligner_set_alignment_free_ends(self.wf, *clamp_span(span, len(p), len(t)))
        return super().align(p, t)


def wfa2_affine2p_endsfree(pairs, spans, pens):
    """-> (scores, cigars) of WFA2 for every (pattern, text) under its span and penalties."""
    aligners, scores, cigars = {}, [], []
    try:
        for (p, t), span, pen in zip(pairs, spans, pens):
            al = aligners.get(tuple(pen)) or aligners.setdefault(tuple(pen), Wfa2Affine2pEndsFree(pen))
            s, c = al.align(p, t, span)
            scores.append(s)
            cigars.append(c)
    finally:
        for al in aligners.values():
            al.close()
    return np.array(scores, dtype=np.int32), cigars


def dp_affine2p_endsfree_score(p, t, pen, span):
    """Optimal ends-free score: match 0, mismatch x, a gap of n bases min(o1 + n e1, o2 + n e2); bytes compared as they are."""
    x, o1, e1, o2, e2 = pen
    plen, tlen = len(p), len(t)
    pb, pe, tb, te = clamp_span(span, plen, tlen)
    INF = 1 << 40
    P = np.frombuffer(bytes(p), dtype=np.uint8)
    T = np.frombuffer(bytes(t), dtype=np.uint8)
    idx = np.arange(tlen + 1, dtype=np.int64)

    def with_insertions(base):
        out = base
        for o, e in ((o1, e1), (o2, e2)):
            run = np.minimum.accumulate(base + o - e * idx)
            ins = np.full(tlen + 1, INF, dtype=np.int64)
            ins[1:] = run[:-1] + e * idx[1:]
            out = np.minimum(out, ins)
        return out

    base = np.full(tlen + 1, INF, dtype=np.int64)
    base[:tb + 1] = 0                     # free starts on the first row
    H = with_insertions(base)
    D1 = np.full(tlen + 1, INF, dtype=np.int64)
    D2 = D1.copy()
    best = int(H[tlen]) if plen <= pe else INF
    for i in range(1, plen + 1):
        D1 = np.minimum(H + o1 + e1, D1 + e1)
        D2 = np.minimum(H + o2 + e2, D2 + e2)
        base = np.minimum(D1, D2)
        base[1:] = np.minimum(base[1:], H[:-1] + np.where(T == P[i - 1], 0, x))
        if i <= pb:
            base[0] = 0                   # free starts on the first column
        H = with_insertions(base)
        if plen - i <= pe:
            best = min(best, int(H[tlen]))
    return min(best, int(H[tlen - te:].min()))


def check_cigar2p_span(p, t, cigar, pen, span, ends=None):
    """-> (valid, cost): endsfree_ref.check_cigar under two pieces.  Validity is its own; the cost leaves out the free bases of the first
    and the last run -- as many as the span allows, or with ends = (k0, k1) exactly what those diagonals say -- and prices every paid
    run by the cheaper piece."""
    valid, _ = ef.check_cigar(p, t, cigar, (0, 0, 1), span, ends)
    items = parse_cigar(cigar)
    if not valid or not items:
        return valid, 0 if valid else -1
    pb, pe, tb, te = clamp_span(span, len(p), len(t))
    free = [0] * len(items)
    if ends is None:
        n, op = items[0]
        free[0] = min(n, tb if op == "I" else pb if op == "D" else 0)
        n, op = items[-1]
        free[-1] += min(n - (free[0] if len(items) == 1 else 0), te if op == "I" else pe if op == "D" else 0)
    else:
        free[0] += abs(int(ends[0]))
        free[-1] += abs(int(ends[1]) - (len(t) - len(p)))
    cost = sum(pen[0] * n if op == "X" else a2.gap_cost(n - f, pen) if op in "ID" and n > f else 0 for (n, op), f in zip(items, free))
    return valid, cost


def make_set(name):
    """-> (pairs, spans, pens) of a golden set."""
    pairs, spans, pens = [], [], []
    if name in ("small", ONE_SET):
        pairs = ef.make_set("small")[0][:200]
        spans = [ef.SMALL_SPANS[i % 9] if name == "small" else ONE_SPAN for i in range(200)]
        pens = [a2.PENS[i % 6] if name == "small" else ONE_PEN for i in range(200)]
    elif name == "wide":
        rng = Rng(20261101)
        for w in WIDE_WIDTHS:
            for j in range(3):
                pbf = ((w - 1) // 2, w - 1, 0)[j]
                tbf = w - 1 - pbf
                core = rng.seq(rng.integer(1100, 1150))
                lead_p, lead_t = rng.seq(rng.integer(0, min(pbf, 100) + 1)), rng.seq(rng.integer(0, min(tbf, 100) + 1))
                pairs.append((lead_p + core, lead_t + rng.mutate(core, 0.03) + rng.seq(rng.integer(0, 20))))
                spans.append((pbf, 5, tbf, 30))
                pens.append(a2.DEFAULT_PEN)
    elif name == "gaps":
        rng = Rng(20261102)
        for i in range(36):
            pen = GAPS_PENS[i % 2]
            n = a2.crossover(pen) + (i // 2) % 3 - 1
            where, insert = ("mid", "begin", "end")[(i // 6) % 3], (i // 18) % 2 == 0
            read = rng.seq(rng.integer(560, 640))
            noisy = rng.mutate(read, 0.01)
            if where == "mid":
                body = a2._plant(rng, noisy, n, True)
                lead, tail = rng.seq(rng.integer(0, GAPS_FREE + 1)), rng.seq(rng.integer(0, GAPS_FREE + 1))
            else:      # n bases more than the free ones stick out at that end
                body = noisy
                lead = rng.seq(GAPS_FREE + n if where == "begin" else rng.integer(0, GAPS_FREE + 1))
                tail = rng.seq(GAPS_FREE + n if where == "end" else rng.integer(0, GAPS_FREE + 1))
            # (insert: the text is the longer side and its ends are free; else the pattern)
            pairs.append((read, lead + body + tail) if insert else (lead + body + tail, read))
            spans.append((0, 0, GAPS_FREE, GAPS_FREE) if insert else (GAPS_FREE, GAPS_FREE, 0, 0))
            pens.append(pen)
    elif name == "ties":
        rng = Rng(20261103)
        for i in range(16):
            p = rng.seq(rng.integer(40, 81))
            pairs.append((p, rng.mutate(p * rng.integer(3, 6), 0.02 if i % 4 else 0.0)))
            spans.append((0, 0, 1000, 1000))
            pens.append(a2.DEFAULT_PEN)
    elif name == LONG_SET:
        rng = Rng(20261104)
        p = rng.seq(33500)
        pairs.append((p, rng.seq(70) + a2._plant(rng, rng.mutate(p, 0.005), 300, True) + rng.seq(55)))
        spans.append((0, 0, 100, 100))
        pens.append(a2.DEFAULT_PEN)
    else:
        raise ValueError(name)
    return pairs, spans, pens


def golden_path(name):
    return os.path.join(ef.GOLDEN, f"affine2p_ef.{name}.alg")


def read_golden(name):
    """-> dict(pairs, spans, pens, scores=int32[n], cigars=[str])"""
    pairs, spans, pens = make_set(name)
    path = golden_path(name)
    with (gzip.open(path + ".gz", "rt") if os.path.exists(path + ".gz") else open(path)) as f:
        rows = [line.rstrip("\n").split("\t") for line in f]
    assert len(rows) == len(pairs)
    return dict(pairs=pairs, spans=spans, pens=pens, scores=np.array([-int(s) for s, _ in rows], dtype=np.int32),
                cigars=["" if c == "*" else c for _, c in rows])


def groups(g):
    """Indices of a golden set by (penalties, span): one device call each."""
    out = {}
    for i, key in enumerate(zip(g["pens"], g["spans"])):
        out.setdefault(key, []).append(i)
    return out


def budget_groups():
    """The groups of test 5: pairs of `small` and `gaps` that share (penalties, span, golden score) -> [((pen, span), score, set, indices)]."""
    import math
    keys, scores, where = [], [], []
    for name in ("small", "gaps"):
        g = read_golden(name)
        keys += [(name,) + k for k in zip(g["pens"], g["spans"])]
        scores += [int(s) for s in g["scores"]]
        where += list(range(len(g["scores"])))
    chosen = ef.sweep_budget_groups(keys, scores, lambda k: math.gcd(*k[1]), 20261105, limit=32)
    return [(k[1:], s, k[0], [where[i] for i in idx]) for k, s, idx in chosen]


if __name__ == "__main__":      # the golden writer: WFA2's answers (run where oracle/_ref is built)
    for name in SETS + (ONE_SET, LONG_SET):
        pairs, spans, pens = make_set(name)
        scores, cigars = wfa2_affine2p_endsfree(pairs, spans, pens)
        text = "".join(f"{-int(s)}\t{c or '*'}\n" for s, c in zip(scores, cigars))
        if len(text) > (256 << 10):
            with gzip.GzipFile(golden_path(name) + ".gz", "wb", mtime=0) as f:
                f.write(text.encode())
        else:
            with open(golden_path(name), "w") as f:
                f.write(text)
        print(name, len(pairs), "pairs, largest score", int(scores.max()))
    bg = budget_groups()
    covered = {k[0] for k, _, _, _ in bg}
    print("budget groups:", len(bg), "penalty sets:", sorted(covered))
    assert len(bg) >= 24 and all(pen in covered for pen in GAPS_PENS), "adjust the sets, not the cap"
