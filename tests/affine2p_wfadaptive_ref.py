"""Ground truth for the wf-adaptive heuristic under two-piece penalties (WFA2's gap_affine_2p with its default strategy) -- test
infrastructure only.  An affine2p_ref.Wfa2Affine2p aligner whose heuristic is set per pair, as wfadaptive_ref.Wfa2Adaptive does; the
pairs by the deterministic recipes of endsfree_ref.Rng and wfadaptive_ref._planted; WFA2's answers in tests/golden/affine2p_ad.<set>.alg.
The heuristic is deterministic: score AND CIGAR are the ground truth, byte for byte."""
import ctypes as C
import os

import numpy as np

from affine2p_ref import Wfa2Affine2p
from endsfree_ref import Rng
from wfadaptive_ref import make_set as wa_make_set
from wfadaptive_ref import _planted, groups  # noqa: F401  (groups: indices of a set by (heuristic, penalties), one device call each)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SETS = ("small", "indel", "long")
HEURS = ((10, 50, 1), (10, 10, 1), (4, 5, 3), (1, 0, 1))
# WFA2's defaults; another concave pair; a common factor of 2; equal pieces
PENS = ((4, 6, 2, 24, 1), (2, 4, 2, 12, 1), (4, 6, 2, 24, 2), (3, 8, 2, 8, 2))
DEFAULT_PEN = PENS[0]
MIN_ABOVE = {"small": 10, "indel": 0, "long": 2}      # pairs whose heuristic score must lie above the two-piece optimum


def wfa2_answers(pairs, heurs, pens):
    """-> (scores, cigars) of WFA2 for every (pattern, text), heuristic (None: exact), penalties."""
    aligners, scores, cigars = {}, [], []
    try:
        for (p, t), heur, pen in zip(pairs, heurs, pens):
            al = aligners.get(tuple(pen))
            if al is None:
                al = aligners[tuple(pen)] = Wfa2Affine2p(pen)
                al.lib.wavefront_aligner_set_heuristic_wfadaptive.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
                al.lib.wavefront_aligner_set_heuristic_wfadaptive.restype = None
            if heur is None:
                al.lib.wavefront_aligner_set_heuristic_none(al.wf)
            else:
                al.lib.wavefront_aligner_set_heuristic_wfadaptive(al.wf, *[int(v) for v in heur])
            s, c = al.align(p, t)
            scores.append(s)
            cigars.append(c)
    finally:
        for al in aligners.values():
            al.close()
    return np.array(scores, dtype=np.int32), cigars


#   small   the first 200 pairs of wfadaptive_ref's `small` (0-300 bases: half related at ~7 %, half unrelated; an empty pattern, an empty
#           text, an identical pair; a few with N / IUPAC bytes).  Pair i runs under HEURS[i % 4] and PENS[(i // 4) % 4]: every combination.
#   indel   the first 32 pairs of wfadaptive_ref's `indel` (~1 kbp at 5 % with one planted 60-base indel, beyond the crossover of 18: I2 /
#           D2 carry the path and get equated), all under (4,5,3): two of three cut-off calls equate without cutting.  PENS[i % 4].
#   long    4 pairs of 5 kbp at 10 % with a 150-base indel, under (10,10,1) and (64,20,1) by turns, default penalties: the ring
#           outgrows LDS (tier 3).  The first seed after 20261102 under which WFA2 alone leaves the optimum on two pairs.
def make_set(name):
    """-> (pairs, heuristics, pens) of a golden set."""
    if name == "small":
        return wa_make_set("small")[0][:200], [HEURS[i % 4] for i in range(200)], [PENS[(i // 4) % 4] for i in range(200)]
    if name == "indel":
        return wa_make_set("indel")[0][:32], [(4, 5, 3)] * 32, [PENS[i % 4] for i in range(32)]
    assert name == "long"
    rng = Rng(20261104)
    return [_planted(rng, 5000, 0.10, 150, i < 2) for i in range(4)], [(10, 10, 1), (64, 20, 1)] * 2, [DEFAULT_PEN] * 4


def golden_path(name):
    return os.path.join(GOLDEN, f"affine2p_ad.{name}.alg")


def write_golden(name, scores, cigars):
    with open(golden_path(name), "w") as f:
        for s, c in zip(scores, cigars):
            f.write(f"{-int(s)}\t{c or '*'}\n")


def read_golden(name):
    """-> dict(pairs=[(pattern, text) bytes], heurs=[3-tuples], pens=[5-tuples], scores=int32[n], cigars=[str])"""
    pairs, heurs, pens = make_set(name)
    scores, cigars = [], []
    with open(golden_path(name)) as f:
        for line in f:
            s, c = line.rstrip("\n").split("\t")
            scores.append(-int(s))
            cigars.append("" if c == "*" else c)
    assert len(pairs) == len(scores)
    return dict(pairs=pairs, heurs=heurs, pens=pens, scores=np.array(scores, dtype=np.int32), cigars=cigars)
