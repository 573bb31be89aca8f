"""The sets of the tier-5 span tests (short_span_ref.py) without a GPU: every line of tests/golden/endsfree.short_*.alg[.gz] against the plain
dynamic program, check_cigar and -- where the reference library is built -- WFA2 live; the model's answers for the metric sets against
their dynamic program; and what each set claims to exercise: the lanes plan_tier's rule gives every call, the shares of pairs within
and over the budget, the shapes in the mix.  A set that stops exercising what it claims fails here, not silently on the GPU."""
import numpy as np
import pytest

import endsfree_ref as er
import linear_endsfree_ref as ler
import linear_ref as lr
import oracle_lib
import short_span_ref as ssr


@pytest.mark.parametrize("name", ["short_sweep", "short_mixed", "short_long", "short_tiny"])
def test_fixture_is_wfa2(name):
    fx = ssr.read_fixture(name)
    for pen, span, pairs in ssr.affine_sets()[name]:
        gold = fx[(pen, span)]
        assert len(gold) == len(pairs)
        for (p, t), (score, cigar) in zip(pairs, gold):
            assert score == er.dp_endsfree_score(p, t, pen, span), (name, pen, span, p, t)
            assert er.check_cigar(p, t, cigar, pen, span) == (True, score), (name, pen, span, p, t, cigar)
        if oracle_lib.have_ref():
            s, c = er.wfa2_endsfree(pairs, [span] * len(pairs), [pen] * len(pairs))
            assert (list(s), c) == ([g[0] for g in gold], [g[1] for g in gold]), (name, pen, span)


def _model_is_the_dp(pen, span, pairs, ref):
    x, g = lr.pens_of(pen)
    for (p, t), (score, cigar, ends) in zip(pairs, ref):
        assert score == ler.dp_linear_endsfree_score(p, t, x, g, span), (pen, span, p, t)
        assert ler.check_cigar_linear_span(p, t, cigar, pen, span, ends=ends) == (True, score), (pen, span, p, t, cigar, ends)


@pytest.mark.parametrize("family", ["affine", "metric"])
def test_sweep_sets(family):
    """Every penalty set the tables hold; per set 16 lanes under its budget, two thirds of the pairs within it and one over; the planted
    gaps are gaps in the reference's CIGAR (M, I and D carry the path), the gaps at the ends continue a free run."""
    sets = ssr.sweep_set(family)
    if family == "affine":
        assert len(set(ssr.AFFINE_PENS)) == len(ssr.AFFINE_PENS) == sum(1 for e in range(1, 5) for x in range(1, 9) for oe in range(e, 9) if np.gcd.reduce([x, oe - e, e]) == 1)
        assert all(ssr.reduced(pen)[:3] in ssr.AFFINE_PENS and ssr.reduced(pen)[3] > 1 for pen in ssr.FACTOR_PENS)
        fx = ssr.read_fixture("short_sweep")
    else:
        assert len(sets) == 2 + 32
    assert all(v > 0 for v in ssr.SWEEP_SPAN)
    for pen, pairs in sets:
        ref = fx[(pen, ssr.SWEEP_SPAN)] if family == "affine" else ssr.model(pen, ssr.SWEEP_SPAN, pairs, "sweep")
        if family == "metric":
            _model_is_the_dp(pen, ssr.SWEEP_SPAN, pairs, ref)
        scores = [r[0] for r in ref]
        budget = ssr.sweep_budget(pen, scores)
        assert ssr.lanes(pen, ssr.SWEEP_SPAN, budget, pairs) == 16, pen
        within = sum(1 for s in scores if s <= budget)
        assert 3 * within >= 2 * len(pairs) and within < len(pairs), (pen, budget, scores)
        # (the re-run of the pairs over the budget stays on tier 5: main_launch_tier == 5 is asserted in every call of the sweep)
        assert ssr.tier5_pairs(pen, ssr.SWEEP_SPAN, budget, pairs, scores) == (len(pairs), len(pairs) - within), pen
        x, o, e, f = ssr.reduced(pen)
        # M, I and D carry the path of some pair within the budget: a gap that is not a run at either end of the CIGAR, and a mismatch
        # where two gaps are not cheaper; the trailing run of pairs 8 and 10 is longer than the free base
        inside = [[op for _, op in er.parse_cigar(r[1])[1:-1]] for r in ref if r[0] <= budget]
        assert any("I" in ops for ops in inside) and any("D" in ops for ops in inside), pen
        assert any("X" in ops for ops in inside) or x is None or x >= 2 * (o + e), pen
        assert ref[8][1].endswith("3I") and ref[8][0] == (o + 2 * e) * f, (pen, ref[8])
        assert ref[10][1].endswith("3D") and ref[10][0] == (o + 2 * e) * f, (pen, ref[10])
        assert scores[0] == scores[13] == 0 and scores[1] > 0


@pytest.mark.parametrize("family", ["affine", "metric"])
def test_mixed_sets(family):
    """Every call plans the lanes it names; among ACGT pairs at least a quarter within the budget and a tenth over it; the count leaves
    the last wavefront partial; the shapes the mix promises are there, neighbours in the list differ."""
    pairs = ssr.mixed_pairs()
    assert len(pairs) == ssr.MIXED_N and ssr.MIXED_N % 4 and ssr.MIXED_N32 % 2 and (ssr.MIXED_N + 3) // 4 > 512 < min((ssr.MIXED_N32 + 1) // 2, ssr.MIXED_N64)
    raw = [ssr.raw_pair(p, t) for p, t in pairs]
    assert 0.005 * len(pairs) <= sum(raw) <= 0.02 * len(pairs) and any(raw[:ssr.MIXED_N64])
    lens = {len(s) for pair in pairs for s in pair}
    assert {0, 1, 15, 16, 17, 31, 32, 33} <= lens and max(lens) <= 60 + 2 * 8 + 8
    assert sum(1 for p, t in pairs if p == t and len(p) >= 8) >= 100 and sum(1 for p, t in pairs if not p and not t) >= 1
    assert sum(1 for p, t in pairs if not p or not t) >= 30 and sum(1 for p, t in pairs if len(p) == 1 or len(t) == 1) >= 30
    fx = ssr.read_fixture("short_mixed") if family == "affine" else None
    for span, want_lanes, n, budgets in ssr.MIXED_CALLS:
        for pen in (ssr.MIXED_AFFINE if family == "affine" else ssr.MIXED_METRIC):
            ref = fx[(pen, span)] if family == "affine" else ssr.model(pen, span, pairs[:n], "mixed")
            if family == "metric":
                _model_is_the_dp(pen, span, pairs[:n], ref)
            scores = np.array([r[0] for r, rw in zip(ref, raw) if not rw])
            assert ssr.lanes(pen, span, budgets[pen], pairs[:n]) == want_lanes, (span, pen)
            within = int((scores <= budgets[pen]).sum())
            assert within >= 0.25 * len(scores) and len(scores) - within >= 0.10 * len(scores), (span, pen, within, len(scores))
            # neighbours differ: of any four pairs in a row (a 16-lane wavefront) seldom all are on one side of the budget
            side = scores <= budgets[pen]
            quads = [side[i:i + 4] for i in range(0, len(side) - 3, 4)]
            assert sum(1 for q in quads if q.any() and not q.all()) >= len(quads) // 4, (span, pen)
            assert 0 in scores and scores.max() > 2 * budgets[pen]


def test_long_set():
    """16 lanes under either budget; every length enters a tail loop of the staging (ASCII: words beyond 16, packed: beyond 32); the two
    pairs whose only edit lies in a tail word; most pairs within the budget, every eighth over it."""
    pairs = ssr.long_pairs()
    assert len(pairs) == ssr.LONG_N and {len(p) for p, _ in pairs} == set(ssr.LONG_LENGTHS)
    words = lambda n: (n + 15) // 16 + 1      # noqa: E731 (the kernel's words_of)
    assert words(240) == 16 and words(241) == 17 and words(496) == 32 and words(497) == 33 and all(words(len(p)) > 16 for p, _ in pairs)
    gold = ssr.read_fixture("short_long")[((2, 3, 1), ssr.LONG_SPAN)]
    edit = ssr.model(lr.EDIT, ssr.LONG_SPAN, pairs, "long")
    _model_is_the_dp(lr.EDIT, ssr.LONG_SPAN, pairs, edit)
    assert gold[ssr.LONG_TAIL_PATTERN] == (2, "2I520M1X8M3I") and gold[ssr.LONG_TAIL_TEXT] == (4, "4I517M1I12M1I")
    for pen, ref in (((2, 3, 1), gold), (lr.EDIT, edit)):
        budget = ssr.LONG_BUDGET[pen]
        assert ssr.lanes(pen, ssr.LONG_SPAN, budget, pairs) == 16 and ssr.lanes(pen, ssr.LONG_SPAN, budget + 1, pairs) == 32
        over = [i for i, r in enumerate(ref) if r[0] > budget]
        assert over == list(range(7, ssr.LONG_N, 8)), (pen, over)
        assert all(r[0] > 0 for r in ref)


def test_tiny_set():
    """961 ordered pairs over {A, C} and 960 with one G; the bound clamps to the nine diagonals of the longest pair, so 16 lanes whatever the span and the budget; the
    model against its dynamic program under every span."""
    pairs = ssr.tiny_pairs()
    assert len(pairs) == ssr.TINY_N and len(set(pairs[:961])) == 961 and max(len(s) for pair in pairs for s in pair) == 4
    assert not any(b"G" in p + t for p, t in pairs[:961]) and all((p + t).count(b"G") == 1 for p, t in pairs[961:])
    assert any(b"G" in p for p, _ in pairs[961:]) and any(b"G" in t for _, t in pairs[961:])
    for pen in ssr.TINY_AFFINE + ssr.TINY_METRIC:
        for span in ssr.TINY_SPANS:
            assert ssr.lanes(pen, span, 1000, pairs) == 16
    assert set(ssr.TINY_WIDE_SPANS) <= set(ssr.TINY_SPANS)
    for pen in ssr.TINY_METRIC:
        for span in ssr.TINY_SPANS:
            _model_is_the_dp(pen, span, pairs, ssr.model(pen, span, pairs, "tiny"))


def test_fixture_bytes():
    import os
    total = sum(os.path.getsize(ssr.fixture_path(name)) for name in ssr.affine_sets())
    assert total < (512 << 10), total
