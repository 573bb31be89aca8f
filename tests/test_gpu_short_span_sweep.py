"""Tier 5 under an ends-free span, every entry of the penalty tables: each (x, o, e) wfa_short_supported takes and that the library can
reach (no common factor: it divides one out first), a few with a common factor that must land on the reduced entry, and every metric
wfa_short_lin_supported takes -- short_span_ref.sweep_set.  Per penalty set nineteen pairs under one span with all four sides non-zero
and a budget that plans 16 lanes; twelve calls: score-only and with CIGARs, from ASCII and from packed words, on 16 lanes as planned and
on 32 and 64 through tuning.waves_per_simd.  Gap-affine against WFA2's bytes (tests/golden/endsfree.short_sweep.alg.gz), the metrics against
the model; test_short_span_cpu.py pins both and asserts what the sets exercise.

main_launch_tier is the call's longest launch.  In every set the re-run of the pairs over the budget (four times the budget) still fits
64 lanes, so every pair of every call finishes on tier 5 (test_short_span_cpu.py asserts that of the sets): pairs_tier[5] is the number
of pairs and main_launch_tier is 5 in every call."""
import pytest

import short_span_ref as ssr
import wfagpu

pytestmark = pytest.mark.gpu


def _sweep(sets, fixture):
    aligners = {(ln, nfp): wfagpu.DeviceAligner(0, no_fused_pack=nfp, **({"waves_per_simd": ln} if ln != 16 else {}))
                for ln in (16, 32, 64) for nfp in (0, 1)}
    try:
        for pen, pairs in sets:
            ref = fixture[(pen, ssr.SWEEP_SPAN)] if fixture else ssr.model(pen, ssr.SWEEP_SPAN, pairs, "sweep")
            scores = [r[0] for r in ref]
            budget = ssr.sweep_budget(pen, scores)
            assert ssr.lanes(pen, ssr.SWEEP_SPAN, budget, pairs) == 16, pen
            on5, over = ssr.tier5_pairs(pen, ssr.SWEEP_SPAN, budget, pairs, scores)
            assert 0 < over == sum(1 for s in scores if s > budget) <= len(pairs) // 3, pen
            buf, meta = wfagpu.layout_pairs(pairs)
            batch = aligners[(16, 0)].upload(buf, meta)
            # the edge of the rule itself: the largest budget that plans 16 lanes does, the next one that widens the bound plans 32
            for edge, ln in ((ssr.sweep_cap(pen), 16), (ssr.sweep_cap(pen) + ssr.reduced(pen)[2] * ssr.reduced(pen)[3], 32)):
                assert ssr.lanes(pen, ssr.SWEEP_SPAN, edge, pairs) == ln, (pen, edge)
                st = ssr.check_call(aligners[(16, 0)], batch, pairs, pen, ssr.SWEEP_SPAN, edge, False, ref, ("sweep", pen, "edge", ln))
                assert st.waves_per_simd_tier0 == ln and st.pairs_retried == sum(1 for s in scores if s > edge), (pen, edge, st.waves_per_simd_tier0)
            for (ln, nfp), al in aligners.items():
                for cigar in (False, True):
                    tag = ("sweep", pen, ln, nfp, cigar)
                    st = ssr.check_call(al, batch, pairs, pen, ssr.SWEEP_SPAN, budget, cigar, ref, tag)
                    assert st.waves_per_simd_tier0 == ln, (tag, st.waves_per_simd_tier0)
                    assert st.pairs_retried == over and st.pairs_raw == 0, (tag, st.pairs_retried, over)
                    assert st.pairs_tier[5] == on5 == len(pairs), (tag, list(st.pairs_tier), on5)
                    assert st.main_launch_tier == 5, (tag, st.main_launch_tier)
    finally:
        for al in aligners.values():
            al.close()


@pytest.mark.parametrize("e", [1, 2, 3, 4])
def test_gap_affine_tables(e):
    """The translation unit of one gap extension: every (x, o) of its tables, and the penalties with a common factor that reduce to it."""
    sets = [(pen, pairs) for pen, pairs in ssr.sweep_set("affine") if ssr.reduced(pen)[2] == e]
    assert len(sets) >= 8 * (9 - e) // 2
    _sweep(sets, ssr.read_fixture("short_sweep"))


@pytest.mark.parametrize("g", [1, 2, 3, 4])
def test_metric_tables(g):
    """Edit and indel (g = 1) and every ("linear", x, g)."""
    sets = [(pen, pairs) for pen, pairs in ssr.sweep_set("metric") if (pen[2] if pen[0] == "linear" else 1) == g]
    assert len(sets) == (10 if g == 1 else 8)
    _sweep(sets, None)
