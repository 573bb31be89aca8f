#!/usr/bin/env python3
"""Regenerates tests/golden/affine2p.{small,gaps,ties,small_default,long,sweep}.alg: WFA2's gap_affine_2p score and CIGAR (the reference's WFA2
compiled in place by oracle/Makefile; run where oracle/_ref exists) for the pairs and penalties that tests/affine2p_ref.py: make_set
rebuilds -- the sets are described there.  Fixtures are DATA."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "tests"))

import affine2p_ref as a2  # noqa: E402
import oracle_lib  # noqa: E402


def main():
    oracle_lib.build()
    assert oracle_lib.have_ref(), "oracle/_ref not built (reference tree missing?)"
    total = 0
    for name in a2.SETS + (a2.ONE_PEN_SET, a2.LONG_SET, a2.SWEEP_SET):
        pairs, pens = a2.make_set(name)
        scores, cigars = a2.wfa2_affine2p(pairs, pens)
        a2.write_golden(name, scores, cigars)
        total += os.path.getsize(a2.golden_path(name))
        print(name, len(pairs), "pairs, largest score", int(scores.max()))
    print("bytes:", total)
    assert total < (1 << 20)


if __name__ == "__main__":
    main()
