"""Tier 5 under an ends-free span, exhaustively on tiny pairs: all 961 ordered pairs of strings over {A, C} of 0 to 4 bases, and each again
with one base replaced by a G (a mismatch against a third letter), under six spans -- everything free, either sequence's ends, a little
of each, crossed ends, nothing.  Nearly every cell of these alignments sits next to a sequence end and an end diagonal, and many end diagonals tie: this is where nulling an I / D value as soon as it passes the end of
its diagonal (short_kernel_body.inc, step) would differ from WFA2's trimming if the argument there were wrong.  Gap-affine against WFA2's
bytes (tests/golden/endsfree.short_tiny.alg.gz: an e = 1 set, a zero opening, rings at e = 2 and e = 3), the metrics against the model.
One call per (penalties, span) under a budget above the call's largest score: the bound clamps to the nine diagonals of the longest
pair, 16 lanes, every pair finishes on tier 5; two of the spans run again on 64 lanes, where the neighbours of lanes 0 and 63 are NULL
next to live end lanes."""
import pytest

import short_span_ref as ssr
import wfagpu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("pen", ssr.TINY_AFFINE + ssr.TINY_METRIC, ids=lambda p: "_".join(map(str, p)))
def test_every_tiny_pair(pen):
    pairs = ssr.tiny_pairs()
    fixture = None if ssr.is_metric(pen) else ssr.read_fixture("short_tiny")
    buf, meta = wfagpu.layout_pairs(pairs)
    aligners = {(ln, nfp): wfagpu.DeviceAligner(0, no_fused_pack=nfp, **({"waves_per_simd": ln} if ln != 16 else {})) for ln in (16, 64) for nfp in (0, 1)}
    try:
        batch = next(iter(aligners.values())).upload(buf, meta)
        for span in ssr.TINY_SPANS:
            ref = fixture[(pen, span)] if fixture else ssr.model(pen, span, pairs, "tiny")
            budget = max(r[0] for r in ref) + 1
            assert ssr.lanes(pen, span, budget, pairs) == 16
            for (ln, nfp), al in aligners.items():
                if ln == 64 and span not in ssr.TINY_WIDE_SPANS:
                    continue
                for cigar in (False, True):
                    tag = ("tiny", pen, span, ln, nfp, cigar)
                    st = ssr.check_call(al, batch, pairs, pen, span, budget, cigar, ref, tag)
                    assert st.pairs_tier[5] == len(pairs) and st.pairs_retried == 0 and st.pairs_raw == 0, (tag, list(st.pairs_tier), st.pairs_retried)
                    assert st.waves_per_simd_tier0 == ln and st.main_launch_tier == 5, (tag, st.waves_per_simd_tier0, st.main_launch_tier)
    finally:
        for al in aligners.values():
            al.close()
