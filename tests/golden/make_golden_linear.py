#!/usr/bin/env python3
"""Regenerates tests/golden/linear.{small,small_edit,ties,lanes,wide,long,sweep}.alg: WFA2's edit, indel and gap-linear score and CIGAR (the
reference's WFA2 compiled in place by oracle/Makefile; run where oracle/_ref exists) for the pairs and metrics that
tests/linear_ref.py: make_set rebuilds -- the sets are described there.  Fixtures are DATA."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "tests"))

import linear_ref as lr  # noqa: E402
import oracle_lib  # noqa: E402


def main():
    oracle_lib.build()
    assert oracle_lib.have_ref(), "oracle/_ref not built (reference tree missing?)"
    total = 0
    for name in lr.SETS + (lr.LONG_SET, lr.SWEEP_SET):
        pairs, metrics = lr.make_set(name)
        scores, cigars = lr.wfa2_linear(pairs, metrics)
        if name == "small":
            # the indel metric is not gap-linear (2, 1) under another name: the scores agree, at least a quarter of the CIGARs do not
            idx = [i for i, m in enumerate(metrics) if m == lr.INDEL]
            s21, c21 = lr.wfa2_linear([pairs[i] for i in idx], [("linear", 2, 1)] * len(idx))
            assert all(int(scores[i]) == int(s) for i, s in zip(idx, s21))
            differ = sum(cigars[i] != c for i, c in zip(idx, c21))
            print("indel against linear(2,1):", differ, "of", len(idx), "CIGARs differ")
            assert 4 * differ >= len(idx)
        lr.write_golden(name, scores, cigars)
        total += os.path.getsize(lr.golden_path(name))
        print(name, len(pairs), "pairs, largest score", int(scores.max()))
    print("bytes:", total)
    assert total < (1 << 20)


if __name__ == "__main__":
    main()
