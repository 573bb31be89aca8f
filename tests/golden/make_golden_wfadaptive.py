#!/usr/bin/env python3
"""Regenerates tests/golden/wfadaptive.{small,indel,defaults1k,long,beyond16,small_default,sweep}.alg: WFA2's score and CIGAR under its
wf-adaptive heuristic (the reference's WFA2 compiled in place by oracle/Makefile; run where oracle/_ref exists) for the pairs,
heuristics and penalties that tests/wfadaptive_ref.py: make_set rebuilds -- the sets are described there.  Asserts that the heuristic
changes enough answers in the sets that are meant to show it (wfadaptive_ref.MIN_DIFFERENT).  Fixtures are DATA."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "tests"))

import oracle_lib  # noqa: E402
import wfadaptive_ref as wa  # noqa: E402


def main():
    oracle_lib.build()
    assert oracle_lib.have_ref(), "oracle/_ref not built (reference tree missing?)"
    total = 0
    for name in wa.ALL_SETS + (wa.SWEEP_SET,):
        pairs, heurs, pens = wa.make_set(name)
        scores, cigars = wa.wfa2_wfadaptive(pairs, heurs, pens)
        wa.write_golden(name, scores, cigars)
        total += os.path.getsize(wa.golden_path(name))
        line = f"{name} {len(pairs)} pairs, largest score {int(scores.max())}"
        if name in wa.MIN_DIFFERENT:
            n = wa.count_different(wa.read_golden(name), cigars_too=name == "defaults1k")
            line += f", {n} differ from the exact answer"
            assert n >= wa.MIN_DIFFERENT[name], (name, n)
        print(line)
    print("bytes:", total)
    assert total < (1 << 20)


if __name__ == "__main__":
    main()
