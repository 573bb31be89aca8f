#!/usr/bin/env python3
"""Regenerates tests/golden/affine2p_ad.{small,indel,long}.alg: WFA2's score and CIGAR under gap_affine_2p with the wf-adaptive heuristic
(the reference's WFA2 compiled in place by oracle/Makefile; run where oracle/_ref exists) for the pairs, heuristics and penalties that
tests/affine2p_wfadaptive_ref.py: make_set rebuilds -- the sets are described there.  Asserts that the heuristic bites: WFA2's score
lies above WFA2's own exact two-piece score for at least MIN_ABOVE pairs of a set.  Fixtures are DATA."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "tests"))

import affine2p_wfadaptive_ref as ar  # noqa: E402
import oracle_lib  # noqa: E402


def main():
    oracle_lib.build()
    assert oracle_lib.have_ref(), "oracle/_ref not built (reference tree missing?)"
    total = 0
    for name in ar.SETS:
        pairs, heurs, pens = ar.make_set(name)
        scores, cigars = ar.wfa2_answers(pairs, heurs, pens)
        exact, _ = ar.wfa2_answers(pairs, [None] * len(pairs), pens)
        assert (scores >= exact).all()
        above = int((scores > exact).sum())
        assert above >= ar.MIN_ABOVE[name], (name, above)
        ar.write_golden(name, scores, cigars)
        total += os.path.getsize(ar.golden_path(name))
        print(name, len(pairs), "pairs, largest score", int(scores.max()), "above the optimum:", above)
    print("bytes:", total)
    assert total < (256 << 10)


if __name__ == "__main__":
    main()
