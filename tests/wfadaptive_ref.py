"""Ground truth for the wf-adaptive heuristic (WFA2's default strategy) -- test infrastructure only.

  wfa2_wfadaptive    WFA2 itself, through the reference library that oracle/Makefile compiles in place (oracle/_ref/libwfa2ref.so,
                     optional): wavefront_aligner_set_heuristic_wfadaptive on the aligner behind a ref_new() handle, then ref_run()
  exact_answers      the optimum of every pair, and the exact CIGAR (oracle/liboracle.so: needs no reference)
  make_set / read_golden   the golden sets: pairs rebuilt by a deterministic recipe (endsfree_ref.Rng), WFA2's answers in
                     tests/golden/wfadaptive.<set>.alg

A heuristic is (min_wavefront_length, max_distance_threshold, steps_between_cutoffs).  The heuristic is deterministic, so WFA2's score
AND CIGAR are the ground truth, byte for byte."""
import ctypes as C
import os

import numpy as np

import oracle_lib
from endsfree_ref import Rng, ring_depth, sweep_long, sweep_pairs, sweep_top

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
PENS = ((2, 3, 1), (4, 6, 2), (5, 3, 2))
DEFAULTS = (10, 50, 1)
SMALL_HEUR = ((10, 50, 1), (10, 10, 1), (4, 5, 3), (64, 20, 1))
SETS = ("small", "indel", "defaults1k", "long", "beyond16")
# one more .alg over the pairs of `small`: ALL of them under one heuristic and one set of penalties -- what a whole batch of a
# launch_alignments* call, a command line or a big tiled batch runs under
ONE_SET, ONE_HEUR, ONE_PEN = "small_default", (10, 10, 1), (2, 3, 1)
ALL_SETS = SETS + (ONE_SET,)
# pairs of a set whose heuristic answer must differ from the exact one (score above the optimum; defaults1k: score or CIGAR)
MIN_DIFFERENT = {"small": 20, "indel": 5, "long": 2, "defaults1k": 2, "sweep": 10}
# the sweep: the cheapest penalties; e > x; a coprime set; a common factor of 3 (the heuristic counts its steps in scores: the reduced
# search has to cut where WFA2 does); a mismatch deeper than 32; o + e = 65, an M ring of 66 rows: beyond the one-wave tier's 64; o + e = 63, the
# deepest ring of that tier
SWEEP_SET = "sweep"
SWEEP_PENS = ((1, 0, 1), (3, 1, 4), (7, 2, 3), (6, 9, 3), (40, 2, 1), (2, 64, 1), (2, 62, 1))
SWEEP_LONG_PENS = ((7, 2, 3), (2, 64, 1))
# WFA2's defaults; the tightest heuristic there is; three steps between cut-offs; seven; a length few rows of short pairs reach
SWEEP_HEUR = ((10, 50, 1), (1, 0, 1), (4, 5, 3), (2, 1, 7), (64, 20, 2))


class Wfa2Adaptive:
    """One WFA2 aligner (penalties, memory mode) whose heuristic is set per pair."""

    def __init__(self, pen, memory_mode=0):
        self.r = oracle_lib.ref()
        self.lib = C.CDLL(oracle_lib.REF_SO)
        self.lib.wavefront_aligner_set_heuristic_wfadaptive.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        self.lib.wavefront_aligner_set_heuristic_wfadaptive.restype = None
        self.h = self.r.ref_new(pen[0], pen[1], pen[2], memory_mode, 0)
        self.wf = C.c_void_p.from_address(self.h).value      # (the handle's first field: the wavefront_aligner_t*)

    def align(self, p, t, heur):
        self.lib.wavefront_aligner_set_heuristic_wfadaptive(self.wf, *[int(v) for v in heur])
        cap = 2 * (len(p) + len(t)) + 16
        out = C.create_string_buffer(cap)
        s = self.r.ref_run(self.h, p, len(p), t, len(t), out, cap)
        return s, out.value.decode()

    def close(self):
        if self.h:
            self.r.ref_delete(self.h)
            self.h = None


def wfa2_wfadaptive(pairs, heurs, pens, memory_mode=0):
    """-> (scores, cigars) of WFA2 for every (pattern, text), heuristic, penalties."""
    aligners = {}
    scores, cigars = [], []
    try:
        for (p, t), heur, pen in zip(pairs, heurs, pens):
            al = aligners.get(tuple(pen))
            if al is None:
                al = aligners[tuple(pen)] = Wfa2Adaptive(pen, memory_mode)
            s, c = al.align(p, t, heur)
            scores.append(s)
            cigars.append(c)
    finally:
        for al in aligners.values():
            al.close()
    return np.array(scores, dtype=np.int32), cigars


def exact_answers(pairs, pens, cigar=False):
    """-> (optimal scores int32[n], exact CIGARs or None) from the C oracle."""
    scores, cigars = [], []
    for (p, t), pen in zip(pairs, pens):
        s, c, _ = oracle_lib.oracle_pair(p, t, tuple(pen), cigar=cigar)
        scores.append(s)
        cigars.append(c)
    return np.array(scores, dtype=np.int32), (cigars if cigar else None)


# ---- the golden sets -----------------------------------------------------------------------------------------------------------
#   small        400 pairs of 0-300 bases: half related at ~7 %, half unrelated; an empty pattern, an empty text, an identical pair; a
#                dozen with N / IUPAC bytes.  Pair i runs under SMALL_HEUR[i % 4] and PENS[i % 3].
#   indel        64 pairs of ~1 kbp at 5 % with one planted 60-base indel (insertions and deletions by turns), all under (4,5,3)
#   defaults1k   48 unrelated pairs, half 1000/1000 and half 600/900 bases, under (10,50,1) and (10,50,10) by turns
#   long         8 pairs of 5 kbp at 10 % with a 150-base indel, under (10,10,1) and (64,20,1) by turns
#   beyond16     2 pairs of 33.5 kbp at 0.5 %, under (10,50,1)
#   small_default  the pairs of `small`, ALL under (10,10,1) and penalties (2,3,1)
#   sweep        20 short pairs (endsfree_ref.sweep_pairs) per penalty set of SWEEP_PENS, pair i under SWEEP_HEUR[i % 5]; 5 long pairs
#                (sweep_long) under each of SWEEP_LONG_PENS -- M rings of 8 and 66 rows, either side of the one-wave tier's limit --, one per
#                heuristic
def _planted(rng, n, rate, indel, insertion):
    p = rng.seq(n)
    cut = rng.integer(n // 4, 3 * n // 4)
    if insertion:
        t = rng.mutate(p[:cut], rate) + rng.seq(indel) + rng.mutate(p[cut:], rate)
    else:
        t = rng.mutate(p[:cut], rate) + rng.mutate(p[cut + indel:], rate)
    return p, t


def make_set(name):
    """-> (pairs, heuristics, pens) of a golden set."""
    pairs, heurs, pens = [], [], []
    if name == SWEEP_SET:
        # The heuristic changes few answers of short related pairs: the unrelated pairs run to the full length here (they are where it
        # bites), and the seed is the first after 20261004 under which WFA2's score lies above the optimum for ten pairs (MIN_DIFFERENT).
        rng = Rng(20261005)
        for j, pen in enumerate(SWEEP_PENS):
            top = sweep_top(ring_depth(pen))
            for i, pair in enumerate(sweep_pairs(rng, top, j, unrelated=top)):
                pairs.append(pair)
                heurs.append(SWEEP_HEUR[(i + j) % 5])
                pens.append(pen)
        for pen in SWEEP_LONG_PENS:
            for i, pair in enumerate(sweep_long(rng)):
                pairs.append(pair)
                heurs.append(SWEEP_HEUR[i % 5])
                pens.append(pen)
    elif name in ("small", ONE_SET):
        rng = Rng(20260901)
        for i in range(400):
            if i == 9:
                p, t = b"", rng.seq(57)
            elif i == 18:
                p, t = rng.seq(41), b""
            elif i == 27:
                p = rng.seq(173)
                t = p
            elif i % 2 == 0:
                p = rng.seq(rng.integer(20, 301))
                t = rng.mutate(p, 0.07)
            else:
                p, t = rng.seq(rng.integer(1, 301)), rng.seq(rng.integer(1, 301))
            if i % 31 == 5 and len(p) > 4 and len(t) > 4:      # bytes outside ACGT: the byte-compare class
                p = p[:len(p) // 2] + b"N" + p[len(p) // 2 + 1:]
                t = t[:len(t) // 3] + b"NRY"[i % 3:i % 3 + 1] + t[len(t) // 3 + 1:]
            pairs.append((p, t))
            heurs.append(SMALL_HEUR[i % 4] if name == "small" else ONE_HEUR)
            pens.append(PENS[i % 3] if name == "small" else ONE_PEN)
    elif name == "indel":
        rng = Rng(20260932)
        for i in range(64):
            pairs.append(_planted(rng, rng.integer(950, 1051), 0.05, 60, i % 2 == 0))
            heurs.append((4, 5, 3))
            pens.append(PENS[i % 3])
    elif name == "defaults1k":
        rng = Rng(20260923)
        for i in range(48):
            pairs.append((rng.seq(1000), rng.seq(1000)) if i < 24 else (rng.seq(600), rng.seq(900)))
            heurs.append((10, 50, 1) if i % 2 == 0 else (10, 50, 10))
            pens.append(PENS[i % 3])
    elif name == "long":
        rng = Rng(20260924)
        for i in range(8):
            pairs.append(_planted(rng, 5000, 0.10, 150, i % 4 < 2))
            heurs.append((10, 10, 1) if i % 2 == 0 else (64, 20, 1))
            pens.append(PENS[i % 3])
    elif name == "beyond16":
        rng = Rng(20260905)
        for i in range(2):
            p = rng.seq(33500)
            pairs.append((p, rng.mutate(p, 0.005)))
            heurs.append(DEFAULTS)
            pens.append(PENS[i % 3])
    else:
        raise ValueError(name)
    return pairs, heurs, pens


def golden_path(name):
    return os.path.join(GOLDEN, f"wfadaptive.{name}.alg")


def write_golden(name, scores, cigars):
    with open(golden_path(name), "w") as f:
        for s, c in zip(scores, cigars):
            f.write(f"{-int(s)}\t{c or '*'}\n")


def read_golden(name):
    """-> dict(pairs=[(pattern, text) bytes], heurs=[3-tuples], pens=[3-tuples], scores=int32[n], cigars=[str])"""
    pairs, heurs, pens = make_set(name)
    scores, cigars = [], []
    with open(golden_path(name)) as f:
        for line in f:
            s, c = line.rstrip("\n").split("\t")
            scores.append(-int(s))
            cigars.append("" if c == "*" else c)
    assert len(pairs) == len(scores)
    return dict(pairs=pairs, heurs=heurs, pens=pens, scores=np.array(scores, dtype=np.int32), cigars=cigars)


def groups(g):
    """Indices of a golden set by (heuristic, penalties): one device call each."""
    out = {}
    for i, key in enumerate(zip(g["heurs"], g["pens"])):
        out.setdefault(key, []).append(i)
    return out


def count_different(g, cigars_too=False):
    """Pairs of a golden set whose stored (heuristic) score lies above the optimum; cigars_too: or whose CIGAR differs from the exact one."""
    opt, exact_cg = exact_answers(g["pairs"], g["pens"], cigar=cigars_too)
    assert (g["scores"] >= opt).all(), "a heuristic score below the optimum"
    diff = g["scores"] > opt
    if cigars_too:
        diff |= np.array([a != b for a, b in zip(g["cigars"], exact_cg)])
    return int(diff.sum())
