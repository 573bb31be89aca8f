#!/usr/bin/env python3
"""Regenerates tests/golden/linef.{small,small_edit_t50,wide,ties,sweep,long}.alg: WFA2's score and CIGAR under an edit, indel or
gap-linear metric with free ends (the reference's WFA2 compiled in place by oracle/Makefile; run where oracle/_ref exists) for the
pairs, metrics and spans that tests/linear_endsfree_ref.py: make_set rebuilds -- the sets are described there.  Fixtures are DATA."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "tests"))

import endsfree_ref as er  # noqa: E402
import linear_endsfree_ref as ler  # noqa: E402
import linear_ref as lr  # noqa: E402
import oracle_lib  # noqa: E402


def main():
    oracle_lib.build()
    assert oracle_lib.have_ref(), "oracle/_ref not built (reference tree missing?)"
    total = 0
    for name in ler.SETS + (ler.SWEEP_SET, ler.LONG_SET):
        pairs, metrics, spans = ler.make_set(name)
        scores, cigars = ler.wfa2_linear_endsfree(pairs, metrics, spans)
        # how many answers differ from the end-to-end ones under the same metric: a path that ignores the span fails on those
        s_e2e, c_e2e = lr.wfa2_linear(pairs, metrics)
        differ = sum(int(a) != int(b) or c != d for a, b, c, d in zip(scores, s_e2e, cigars, c_e2e))
        if name == "small_edit_t50":
            # the emulation a caller had before: gap-affine (1, 0, 1) under the same span
            s_em, c_em = er.wfa2_endsfree(pairs, spans, [ler.EMULATION_PEN] * len(pairs))
            assert all(int(a) == int(b) for a, b in zip(scores, s_em)), "edit and gap-affine (1,0,1) scores differ under the span"
            agree = sum(c == d for c, d in zip(cigars, c_em))
            print("small_edit_t50 against gap-affine (1,0,1):", agree, "of", len(pairs), "CIGARs agree")
            assert (agree == len(pairs)) == ler.SMALL_EDIT_T50_CIGARS_AGREE, "linear_endsfree_ref.SMALL_EDIT_T50_CIGARS_AGREE is out of date"
        ler.write_golden(name, scores, cigars)
        total += os.path.getsize(ler.golden_path(name))
        print(name, len(pairs), "pairs, largest score", int(scores.max()), "--", differ, "differ from end to end")
    print("bytes:", total)
    assert total < (1 << 20)


if __name__ == "__main__":
    main()
