#!/usr/bin/env python3
"""Regenerates tests/golden/endsfree.{small,wide,ties,small_t50,sweep}.alg: WFA2's ends-free score and CIGAR (the reference's WFA2 compiled
in place by oracle/Makefile; run where oracle/_ref exists) for the pairs, spans and penalties that tests/endsfree_ref.py: make_set
rebuilds -- the sets are described there.  Fixtures are DATA."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "tests"))

import endsfree_ref as ef  # noqa: E402
import oracle_lib  # noqa: E402


def main():
    oracle_lib.build()
    assert oracle_lib.have_ref(), "oracle/_ref not built (reference tree missing?)"
    total = 0
    for name in ef.SETS + (ef.ONE_SPAN_SET, ef.SWEEP_SET):
        pairs, spans, pens = ef.make_set(name)
        scores, cigars = ef.wfa2_endsfree(pairs, spans, pens)
        ef.write_golden(name, scores, cigars)
        total += os.path.getsize(ef.golden_path(name))
        print(name, len(pairs), "pairs")
    print("bytes:", total)
    assert total < (1 << 20)


if __name__ == "__main__":
    main()
