"""Ground truth for two-piece gap-affine alignment (WFA2's gap_affine_2p) -- test infrastructure only.

  wfa2_affine2p      WFA2 itself, through the reference library that oracle/Makefile compiles in place (oracle/_ref/libwfa2ref.so,
                     optional; it exports all of WFA2): a copy of the exported wavefront_aligner_attr_default with the metric and the
                     penalties written into its leading int fields (their layout is fixed by wavefront_attributes.h), then
                     wavefront_aligner_new, wavefront_aligner_set_heuristic_none and ref_run() on a one-pointer handle
  dp_affine2p_score  a plain dynamic program with five matrices (numpy, one vector step per row), independent of WFA2
  check_cigar2p      validity of a CIGAR and its cost, every gap run priced min(o1 + n e1, o2 + n e2)
  make_set / read_golden   the golden sets: pairs rebuilt by a deterministic recipe, WFA2's answers in tests/golden/affine2p.<set>.alg

Penalties are (x, o1, e1, o2, e2): match 0, all five > 0."""
import ctypes as C
import math
import os
import struct

import numpy as np

import oracle_lib
from endsfree_ref import SWEEP_LONG, SWEEP_PAIRS, Rng, parse_cigar, sweep_long, sweep_pairs, sweep_top

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
SETS = ("small", "gaps", "ties")
ONE_PEN_SET, DEFAULT_PEN = "small_default", (4, 6, 2, 24, 1)
LONG_SET = "long"      # (kept out of SETS: the dynamic program would take minutes on it)
# WFA2's defaults; another concave pair; a steep first piece; a common factor of 2; equal pieces; a second piece that never wins
PENS = ((4, 6, 2, 24, 1), (2, 4, 2, 12, 1), (5, 3, 4, 10, 1), (4, 6, 2, 24, 2), (3, 8, 2, 8, 2), (2, 3, 1, 40, 1))
GAP_AFFINE, GAP_AFFINE_2P = 3, 4          # distance_metric_t (wavefront_penalties.h)
ATTR_METRIC_OFF, ATTR_PENS_OFF = 0, 56     # wavefront_aligner_attr_t: distance_metric; affine2p_penalties = {match, x, o1, e1, o2, e2}


def gap_cost(n, pen):
    _, o1, e1, o2, e2 = pen
    return min(o1 + n * e1, o2 + n * e2)


def crossover(pen):
    """The gap length at which both pieces cost the same, (o2 - o1) / (e1 - e2); None where the pieces never cross at a whole length >= 1."""
    _, o1, e1, o2, e2 = pen
    if e1 == e2 or (o2 - o1) % (e1 - e2) or (o2 - o1) // (e1 - e2) < 1:
        return None
    return (o2 - o1) // (e1 - e2)


def _elf_symbol_size(path, name):
    """st_size of a dynamic symbol of a 64-bit little-endian ELF file."""
    with open(path, "rb") as f:
        data = f.read()
    assert data[:6] == b"\x7fELF\x02\x01", "a 64-bit little-endian ELF file"
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    for sec in secs:
        if sec[1] != 11:      # SHT_DYNSYM
            continue
        str_off = secs[sec[6]][4]
        for off in range(sec[4], sec[4] + sec[5], sec[9]):
            st_name, _, _, _, _, st_size = struct.unpack_from("<IBBHQQ", data, off)
            end = data.index(b"\0", str_off + st_name)
            if data[str_off + st_name:end] == name.encode():
                return st_size
    raise KeyError(name)


class Wfa2Affine2p:
    """One WFA2 aligner under gap_affine_2p penalties."""

    def __init__(self, pen):
        self.r = oracle_lib.ref()
        self.lib = C.CDLL(oracle_lib.REF_SO)
        size = _elf_symbol_size(oracle_lib.REF_SO, "wavefront_aligner_attr_default")
        attr = (C.c_char * size).from_buffer_copy((C.c_char * size).in_dll(self.lib, "wavefront_aligner_attr_default"))
        ints = C.cast(attr, C.POINTER(C.c_int))
        assert ints[ATTR_METRIC_OFF // 4] == GAP_AFFINE, "the default attributes start with distance_metric = gap_affine"
        assert tuple(ints[ATTR_PENS_OFF // 4 + i] for i in range(6)) == (0,) + DEFAULT_PEN, "affine2p_penalties at bytes 56-79"
        ints[ATTR_METRIC_OFF // 4] = GAP_AFFINE_2P
        for i, v in enumerate((0,) + tuple(pen)):
            ints[ATTR_PENS_OFF // 4 + i] = int(v)
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
        return s, out.value.decode()

    def close(self):
        if self.wf:
            self.lib.wavefront_aligner_delete(self.wf)
            self.wf = None


def wfa2_affine2p(pairs, pens):
    """-> (scores, cigars) of WFA2 for every (pattern, text) under its penalties."""
    aligners = {}
    scores, cigars = [], []
    try:
        for (p, t), pen in zip(pairs, pens):
            al = aligners.get(tuple(pen))
            if al is None:
                al = aligners[tuple(pen)] = Wfa2Affine2p(pen)
            s, c = al.align(p, t)
            scores.append(s)
            cigars.append(c)
    finally:
        for al in aligners.values():
            al.close()
    return np.array(scores, dtype=np.int32), cigars


def dp_affine2p_score(p, t, pen):
    """Optimal end-to-end score: match 0, mismatch x, a gap of n bases min(o1 + n e1, o2 + n e2); bytes compared as they are.
    Five matrices, a row at a time: H (best), D1 / D2 (the pattern runs on: vertical, one vector step), I1 / I2 (the text runs on:
    horizontal, a running minimum -- a gap opened from a cell that itself ends in a gap of the same kind is never cheaper than one gap,
    the cost of a gap being subadditive)."""
    x, o1, e1, o2, e2 = pen
    plen, tlen = len(p), len(t)
    INF = 1 << 40
    P = np.frombuffer(bytes(p), dtype=np.uint8)
    T = np.frombuffer(bytes(t), dtype=np.uint8)
    idx = np.arange(tlen + 1, dtype=np.int64)

    def horizontal(base, o, e):
        run = np.minimum.accumulate(base + o - e * idx)
        ins = np.full(tlen + 1, INF, dtype=np.int64)
        ins[1:] = run[:-1] + e * idx[1:]
        return ins

    base = np.full(tlen + 1, INF, dtype=np.int64)
    base[0] = 0
    I1, I2 = horizontal(base, o1, e1), horizontal(base, o2, e2)
    H = np.minimum(base, np.minimum(I1, I2))
    D1 = np.full(tlen + 1, INF, dtype=np.int64)
    D2 = np.full(tlen + 1, INF, dtype=np.int64)
    for i in range(1, plen + 1):
        D1 = np.minimum(H + o1 + e1, D1 + e1)
        D2 = np.minimum(H + o2 + e2, D2 + e2)
        base = np.minimum(D1, D2)
        base[1:] = np.minimum(base[1:], H[:-1] + np.where(T == P[i - 1], 0, x))
        I1, I2 = horizontal(base, o1, e1), horizontal(base, o2, e2)
        H = np.minimum(base, np.minimum(I1, I2))
    return int(H[tlen])


def check_cigar2p(p, t, cigar, pen):
    """-> (valid, cost).  valid: the CIGAR is run-length encoded without equal neighbours, covers both whole sequences, M sits on equal
    and X on different bytes.  cost: x per mismatch, min(o1 + n e1, o2 + n e2) per gap run of n bases."""
    x = pen[0]
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
            cost += x * n if op == "X" else 0
        else:
            if op == "I":
                h += n
            else:
                v += n
            cost += gap_cost(n, pen)
    valid &= v == plen and h == tlen
    return bool(valid), cost


# ---- the golden sets -----------------------------------------------------------------------------------------------------------
# The PAIRS of a set are not stored: make_set() rebuilds them, bit for bit on every machine, from the counter-based generator of
# endsfree_ref (Rng).  Stored are WFA2's answers, tests/golden/affine2p.<set>.alg, one "-score<TAB>CIGAR" line per pair like the other
# .alg fixtures ("*": an empty CIGAR); tests/golden/make_golden_affine2p.py writes them.
#   small          400 pairs of 0-300 bases: half of them related at ~6 % error, half unrelated; an empty pattern, an empty text and an
#                  identical pair among them; thirteen hold N / IUPAC bytes (the byte-compare class).  Pair i runs under PENS[i % 6].
#   gaps           48 pairs of 1.1-1.3 kbp (1075-1325 bases: a planted indel of 200 bases spans the range, the noise adds a few) at ~3 % noise with one to three planted indels whose lengths straddle the crossover n* of the
#                  pair's penalties (n* - 1, n*, n* + 1; 12 where the pieces do not cross) or are 63, 64, 65 or 200: both pieces are used,
#                  rows cross lane and wave boundaries.  Pair i runs under PENS[i % 6].
#   ties           32 pairs with a tandem repeat or a homopolymer run from which exactly n* bases are cut (or into which they are put): both
#                  pieces cost the same and the gap can sit anywhere in the repeat -- WFA2's priority order decides the CIGAR.  Penalties
#                  with a whole crossover: PENS[0] (18) and PENS[1] (8), alternating.
#   small_default  the pairs of `small`, ALL under (4,6,2,24,1): a whole call, command line or seam batch under one set.
#   long           2 pairs of 33.5 kbp at ~0.5 % noise with a planted indel of 300 bases, under (4,6,2,24,1): sequences beyond 32766 bases
#                  run on the tier with 32-bit offsets.
GAP_LENGTHS_FIXED = (63, 64, 65, 200)


def _plant(rng, s, n, insert):
    """n bases cut out of s (or put into it) somewhere in its middle half."""
    at = rng.integer(len(s) // 4, 3 * len(s) // 4 - n)
    return s[:at] + rng.seq(n) + s[at:] if insert else s[:at] + s[at + n:]


#   sweep          SWEEP_PAIRS short pairs (endsfree_ref.sweep_pairs) under each of SWEEP_PENS; SWEEP_LONG long pairs (sweep_long) under
#                  each of SWEEP_LONG_PENS, M rings of 64 and 66 rows: either side of the one-wave tier's limit of 64.
SWEEP_SET = "sweep"
# two cheap sets; a common factor of 3; M rings of 64, 65 and 66 rows (max(x, o1 + e1, o2 + e2) + 1); a mismatch deeper than either piece; the
# pieces swapped (the first is the flat one); a second piece that always wins (o2 < o1, e2 < e1); deep I/D rings (e1 = 6, e2 = 5);
# e2 > e1 with o2 = o1 (the second piece never wins).  WFA2 accepts all eleven.
SWEEP_PENS = ((1, 1, 2, 4, 1), (3, 2, 3, 9, 1), (6, 9, 3, 30, 3), (2, 3, 1, 62, 1), (2, 3, 1, 63, 1), (2, 3, 1, 64, 1), (40, 6, 2, 24, 1),
              (4, 24, 1, 6, 2), (4, 6, 2, 3, 1), (5, 2, 6, 20, 5), (2, 1, 1, 1, 3))
SWEEP_LONG_PENS = ((2, 3, 1, 62, 1), (2, 3, 1, 64, 1))


def ring_depth(pen):
    """Rows of the M ring the kernels run: one per score back to the deepest source, max(x, o1 + e1, o2 + e2) below, and the row being
    written -- of the penalties without their common factor, which the library divides out first."""
    x, o1, e1, o2, e2 = pen
    return max(x, o1 + e1, o2 + e2) // math.gcd(*pen) + 1


def make_set(name):
    """-> (pairs, pens) of a golden set."""
    pairs, pens = [], []
    if name == SWEEP_SET:
        rng = Rng(20261002)
        for j, pen in enumerate(SWEEP_PENS):
            pairs += sweep_pairs(rng, sweep_top(ring_depth(pen)), j)
            pens += [pen] * SWEEP_PAIRS
        for pen in SWEEP_LONG_PENS:
            pairs += sweep_long(rng)
            pens += [pen] * SWEEP_LONG
    elif name in ("small", ONE_PEN_SET):
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
            pens.append(PENS[i % 6] if name == "small" else DEFAULT_PEN)
    elif name == "gaps":
        rng = Rng(20260202)
        for i in range(48):
            pen = PENS[i % 6]
            nstar = crossover(pen) or 12
            lengths = (max(nstar - 1, 1), nstar, nstar + 1) + GAP_LENGTHS_FIXED
            # the first indel an insertion or a deletion by turns, every further one whatever brings the text's length back towards the
            # pattern's; the pattern's length centred so that both sequences stay near 1.1-1.3 kbp (a 200-base indel spans that range)
            planted, net = [], 0
            for j in range(1 + i % 3):
                n = lengths[(i // 6 * 3 + 2 * j + i % 6) % len(lengths)]
                insert = (i // 6 + i) % 2 == 0 if j == 0 else net < 0
                planted.append((n, insert))
                net += n if insert else -n
            p = rng.seq(1200 - net // 2 + rng.integer(-10, 11))
            t = rng.mutate(p, 0.03)
            for n, insert in planted:
                t = _plant(rng, t, n, insert)
            pairs.append((p, t))
            pens.append(pen)
    elif name == "ties":
        rng = Rng(20260203)
        for i in range(32):
            pen = PENS[i % 2]
            nstar = crossover(pen)
            unit = rng.seq(1 if i % 4 < 2 else rng.integer(2, 7))
            reps = (nstar + len(unit) - 1) // len(unit) * 2 + rng.integer(2, 6)
            left, right = rng.seq(rng.integer(60, 140)), rng.seq(rng.integer(60, 140))
            long_run, short_run = unit * reps, (unit * reps)[nstar:]
            a, b = left + long_run + right, left + short_run + right
            p, t = (a, b) if i % 8 < 4 else (b, a)
            pairs.append((p, rng.mutate(t, 0.01 if i % 3 == 0 else 0.0)))
            pens.append(pen)
    elif name == LONG_SET:
        rng = Rng(20260205)
        for i in range(2):
            p = rng.seq(33500 + 37 * i)
            pairs.append((p, _plant(rng, rng.mutate(p, 0.005), 300, insert=i == 0)))
            pens.append(DEFAULT_PEN)
    else:
        raise ValueError(name)
    return pairs, pens


def golden_path(name):
    return os.path.join(GOLDEN, f"affine2p.{name}.alg")


def write_golden(name, scores, cigars):
    with open(golden_path(name), "w") as f:
        for s, c in zip(scores, cigars):
            f.write(f"{-int(s)}\t{c or '*'}\n")


def read_golden(name):
    """-> dict(pairs=[(pattern, text) bytes], pens=[5-tuples], scores=int32[n], cigars=[str])"""
    pairs, pens = make_set(name)
    scores, cigars = [], []
    with open(golden_path(name)) as f:
        for line in f:
            s, c = line.rstrip("\n").split("\t")
            scores.append(-int(s))
            cigars.append("" if c == "*" else c)
    assert len(pairs) == len(scores)
    return dict(pairs=pairs, pens=pens, scores=np.array(scores, dtype=np.int32), cigars=cigars)


def groups(g):
    """Indices of a golden set by penalties: one device call each."""
    out = {}
    for i, pen in enumerate(g["pens"]):
        out.setdefault(tuple(pen), []).append(i)
    return out
