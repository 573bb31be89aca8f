#!/usr/bin/env python3
"""Regenerates tests/golden/endsfree.short_{sweep,mixed,tiny}.alg.gz and endsfree.short_long.alg: WFA2's ends-free gap-affine score and CIGAR (the reference's WFA2
compiled in place by oracle/Makefile; run where oracle/_ref exists) for the calls that tests/short_span_ref.py: affine_sets rebuilds --
the sets are described there.  The three large sets are written as gzip of the usual text (as text they would pass the 512 KiB this
script allows itself; zcat shows the lines).  The metric sets have no fixture: the Python model answers them.  Fixtures are DATA."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "tests"))

import endsfree_ref as ef  # noqa: E402
import oracle_lib  # noqa: E402
import short_span_ref as ssr  # noqa: E402


def main():
    oracle_lib.build()
    assert oracle_lib.have_ref(), "oracle/_ref not built (reference tree missing?)"
    total = 0
    for name, calls in ssr.affine_sets().items():
        scores, cigars = [], []
        for pen, span, pairs in calls:
            s, c = ef.wfa2_endsfree(pairs, [span] * len(pairs), [pen] * len(pairs))
            scores += list(s)
            cigars += c
        ssr.write_fixture(name, scores, cigars)
        total += os.path.getsize(ssr.fixture_path(name))
        print(name, len(calls), "calls,", len(scores), "pairs,", os.path.getsize(ssr.fixture_path(name)), "bytes")
    print("bytes:", total)
    assert total < (512 << 10)


if __name__ == "__main__":
    main()
