"""Tier 5 under an ends-free span on batches whose neighbours disagree: 515 to 2051 shuffled pairs per call -- reads in windows at 0 / 3 /
10 %, unrelated, identical, empty, one base, lengths around the packed-word seams, ~1 % holding N / IUPAC bytes -- so that the groups
that share a wavefront finish at score 0, at the budget, run out of it, are empty or are flagged for the byte-compare class, side by
side; and 64 long reads on 16 lanes, whose words beyond the sixteenth (ASCII) and the thirty-second (packed) are staged by the tail loops.
Gap-affine against WFA2's bytes (tests/golden/endsfree.short_mixed.alg.gz, .short_long.alg), the metrics against the model;
test_short_span_cpu.py pins both and asserts the shares, the lanes and the shapes.

The grid (wfa_host.hip): a tier-5 launch takes as many wavefronts as it has work items, up to every wavefront the chip holds --
thousands: a few thousand pairs are one iteration per wavefront, and three on a full grid would take some 100 000 pairs.  So every call
runs twice: as shipped (one iteration, every wavefront's pipeline filled and drained at once) and with tuning.max_blocks_per_cu = 1 (one
wavefront per CU, 256 of them), under which the smallest counts with three iterations per wavefront are used: 2051 pairs on 16 lanes
(513 work items of four pairs on 171 wavefronts), 1027 on 32 lanes (514 items on 172), 515 on 64 (515 on 172) -- the three-stage pipeline
in steady state.  2051 and 1027 pairs leave the last wavefront partial.

The retry rule: what fails runs again under four times the budget, on tier 5 where that still fits 64 lanes.  short_span_ref.tier5_pairs
follows it, so pairs_tier[5] is asserted exactly in every call: the pairs within the budget where the re-run leaves tier 5 -- (2,3,1) under
17 and (0,0,8,8): 68 does not fit --, those within four times the budget where it does not -- (2,3,1) under 11 and (0,0,3,3): 44 fits 64
lanes.  pairs_retried counts the first round's failures of both classes, and the byte-compare class runs its first round under the same
budget: in every call it equals the ACGT pairs over the budget plus the flagged pairs over it -- a pair within the budget that came back
for a wider group would break the equality.  waves_per_simd_tier0 is the first launch's of the class that ran last, so every call runs
again on the ACGT pairs alone, where it is tier 5's and must be the lanes planned."""
import pytest

import linear_ref as lr
import short_span_ref as ssr
import wfagpu

pytestmark = pytest.mark.gpu


def _ref(pen, span, pairs, key):
    name = "short_long" if key == "long" else "short_mixed"
    return ssr.model(pen, span, pairs, key) if ssr.is_metric(pen) else ssr.read_fixture(name)[(pen, span)]


_TUNINGS = ({}, {"no_fused_pack": 1}, {"max_blocks_per_cu": 1}, {"max_blocks_per_cu": 1, "no_fused_pack": 1}, {"min_tier": 1})


def _calls(pairs, pen, span, budget, want_lanes, ref, key):
    """Every tuning, score-only and with CIGARs, on one list of pairs; every counter exact."""
    raw = [ssr.raw_pair(p, t) for p, t in pairs]
    n_raw = sum(raw)
    acgt_scores = [r[0] for r, rw in zip(ref, raw) if not rw]
    on5, over = ssr.tier5_pairs(pen, span, budget, pairs, acgt_scores)
    within = sum(1 for s in acgt_scores if s <= budget)
    assert on5 >= within and over == len(acgt_scores) - within
    assert ssr.lanes(pen, span, budget, pairs) == want_lanes
    # the byte-compare class runs its own first round under the same budget: its pairs over the budget come back as well
    raw_over = sum(1 for r, rw in zip(ref, raw) if rw and r[0] > budget)
    aligners = [(tuning, wfagpu.DeviceAligner(0, **tuning)) for tuning in _TUNINGS]
    try:
        batch = aligners[0][1].upload(*wfagpu.layout_pairs(pairs))      # one upload serves every aligner; all stay open until the end
        for tuning, al in aligners:
            for cigar in (False, True):
                tag = (key, pen, span, len(pairs), tuple(tuning), cigar)
                st = ssr.check_call(al, batch, pairs, pen, span, budget, cigar, ref, tag)
                assert st.pairs_raw == n_raw, (tag, st.pairs_raw, n_raw)
                assert st.pairs_retried == over + raw_over, (tag, st.pairs_retried, over, raw_over)
                if "min_tier" in tuning:
                    assert st.pairs_tier[5] == 0, (tag, list(st.pairs_tier))
                    continue
                assert st.pairs_tier[5] == on5, (tag, list(st.pairs_tier), on5, within)
                # (waves_per_simd_tier0 is the first launch's of the class that ran last: the byte-compare class's where the batch has one)
                assert n_raw or st.waves_per_simd_tier0 == want_lanes, (tag, st.waves_per_simd_tier0)
    finally:
        for _, al in aligners:
            al.close()
    return raw


def _run(pairs, pen, span, budget, want_lanes, ref, key):
    raw = _calls(pairs, pen, span, budget, want_lanes, ref, key)
    if any(raw):
        # the same calls on the ACGT pairs alone (one dropped where they would fill the last wavefront): the first launch's lanes are tier 5's
        keep = [i for i, rw in enumerate(raw) if not rw]
        keep = keep[:len(keep) - (1 if len(keep) % 4 == 0 else 0)]
        _calls([pairs[i] for i in keep], pen, span, budget, want_lanes, [ref[i] for i in keep], key)


@pytest.mark.parametrize("call", range(len(ssr.MIXED_CALLS)))
@pytest.mark.parametrize("pen", ssr.MIXED_AFFINE + ssr.MIXED_METRIC, ids=lambda p: "_".join(map(str, p)))
def test_mixed_batch(pen, call):
    span, want_lanes, n, budgets = ssr.MIXED_CALLS[call]
    pairs = ssr.mixed_pairs()[:n]
    _run(pairs, pen, span, budgets[pen], want_lanes, _ref(pen, span, pairs, "mixed"), "mixed")


@pytest.mark.parametrize("pen", [(2, 3, 1), lr.EDIT], ids=lambda p: "_".join(map(str, p)))
def test_long_reads_on_16_lanes(pen):
    """241 / 273 / 497 / 529 bases under (0, 0, 4, 4) and a budget of 9 (edit: 6): 16 lanes.  529 bases stay on tier 5 with CIGARs -- neither
    seq_words_cap (35 words a sequence: 2240 bytes of LDS for the four pairs' two sets) nor the 40 KiB rule (64 bytes a score) is near.
    Pair 0's only edit is a substitution at base 520 of the pattern, pair 1's an insertion behind base 520 of the text: words the tail
    loops stage on either path."""
    pairs = ssr.long_pairs()
    _run(pairs, pen, ssr.LONG_SPAN, ssr.LONG_BUDGET[pen], 16, _ref(pen, ssr.LONG_SPAN, pairs, "long"), "long")
