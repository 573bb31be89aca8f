"""Ends-free (semi-global) alignment on the GPU: wfagpu_amd_align_device_span, wfagpu_amd_configure_span behind the
launch_alignments* seam and the CLI, against WFA2's ends-free scores and CIGARs (tests/golden/endsfree.*, made by
tests/golden/make_golden_endsfree.py; the sets are described in tests/endsfree_ref.py)."""
import ctypes as C
import math
import os
import random
import subprocess

import numpy as np
import pytest

import endsfree_ref as ef
import wfagpu

pytestmark = pytest.mark.gpu
PKG = os.path.dirname(wfagpu.LIB_PATH)
CLI = os.path.join(PKG, "bin", "wfa.affine.gpu")
INT32_MIN = -(2**31)
# score budgets of the first tier: above every golden score of the set (small: unrelated 300-base pairs under (5,3,2); wide and ties:
# ~5 % of 1.2 kbp), small enough for wide to start on the one-wave tier
MAX_ERROR = {"small": 2000, "wide": 400, "ties": 400}


@pytest.fixture(scope="module")
def sets():
    return {name: ef.read_golden(name) for name in ef.SETS + (ef.ONE_SPAN_SET,)}


def _run_set(al, g, cigar, max_error, only=None):
    """Every (span, penalties) group of a golden set as one call -> scores, cigars, ends in the set's order (only: a subset of indices).
    No pair is skipped: every index must have come back."""
    n = len(g["pairs"])
    scores = np.full(n, -12345, dtype=np.int64)
    cigars = [None] * n
    ends = np.zeros((n, 2), dtype=np.int64)
    seen = 0
    stats = []
    for (span, pen), idx in ef.groups(g).items():
        if only is not None:
            idx = [i for i in idx if i in only]
            if not idx:
                continue
        buf, meta = wfagpu.layout_pairs([g["pairs"][i] for i in idx])
        batch = al.upload(buf, meta)
        s, c, e = al.align(batch, pen, max_error=max_error, compute_cigar=cigar, span=span, fetch_ends=True)
        stats.append(al.stats())
        for j, i in enumerate(idx):
            scores[i] = s[j]
            cigars[i] = c[j] if cigar else None
            ends[i] = e[j]
        seen += len(idx)
    assert seen == (n if only is None else len(only))
    return scores, cigars, ends, stats


def _check_set(g, scores, cigars, ends, cigar, only=None):
    for i in (range(len(g["pairs"])) if only is None else sorted(only)):
        p, t = g["pairs"][i]
        span, pen = g["spans"][i], g["pens"][i]
        where = (i, len(p), len(t), span, pen)
        assert scores[i] == g["scores"][i], where
        pb, pe, tb, te = ef.clamp_span(span, len(p), len(t))
        kend = len(t) - len(p)
        k0, k1 = int(ends[i][0]), int(ends[i][1])
        assert kend - te <= k1 <= kend + pe, where
        if cigar:
            assert cigars[i] == g["cigars"][i], where
            ok, cost = ef.check_cigar(p, t, cigars[i], pen, span, ends=(k0, k1))
            assert ok and cost == scores[i], where + (k0, k1, cigars[i])
        else:
            assert k0 == INT32_MIN, where      # (the start diagonal is the backtrace's to find)


def test_span_of_zeros_is_the_end_to_end_alignment(golden_dir):
    """All four values zero on the reference's 1 kbp pairs: scores and CIGAR bytes of wfagpu_amd_align_device on the same context, and
    ends = (0, tlen - plen)."""
    pairs = wfagpu.read_seq_file(os.path.join(golden_dir, "seq1k.seq"))
    buf, meta = wfagpu.layout_pairs(pairs)
    kend = meta["text_len"].astype(np.int64) - meta["pattern_len"].astype(np.int64)
    al = wfagpu.DeviceAligner(0)
    try:
        batch = al.upload(buf, meta)
        for pen in ((2, 3, 1), (5, 3, 2)):
            gold = -np.loadtxt(os.path.join(golden_dir, f"seq1k.x{pen[0]}o{pen[1]}e{pen[2]}.scores"), dtype=np.int64)
            s0, c0 = al.align(batch, pen, max_error=1000, compute_cigar=True)
            s1, c1, e1 = al.align(batch, pen, max_error=1000, compute_cigar=True, span=(0, 0, 0, 0), fetch_ends=True)
            assert np.array_equal(s0, gold[:len(s0)])
            assert np.array_equal(s1, s0) and c1 == c0
            assert np.array_equal(e1[:, 0], np.zeros(len(pairs))) and np.array_equal(e1[:, 1], kend)
            s2, _, e2 = al.align(batch, pen, max_error=1000, compute_cigar=False, span=(0, 0, 0, 0), fetch_ends=True)
            assert np.array_equal(s2, s0) and np.array_equal(e2[:, 1], kend)
    finally:
        al.close()


@pytest.mark.parametrize("name", ef.SETS)
@pytest.mark.parametrize("cigar", [False, True])
def test_golden_sets(sets, name, cigar):
    """score == WFA2's, CIGAR == WFA2's byte for byte, the diagonals consistent with the CIGAR's free runs."""
    g = sets[name]
    al = wfagpu.DeviceAligner(0)
    try:
        scores, cigars, ends, _ = _run_set(al, g, cigar, MAX_ERROR[name])
        _check_set(g, scores, cigars, ends, cigar)
    finally:
        al.close()


@pytest.mark.parametrize("variant", ["min_tier1", "min_tier2", "min_tier3", "max_error8", "small_arena", "trace_mode1", "trace_mode2",
                                     "trace_mode3", "trace_mode4"])
def test_golden_sets_on_every_path(sets, variant):
    """The same batches forced through the wider tiers, through escalation (a budget of 8: most pairs miss it), through several
    arena-bound passes, and through every mapping of the backtrace: the same bytes."""
    kw, max_error = {}, None
    if variant.startswith("min_tier"):
        kw["min_tier"] = int(variant[-1])
    elif variant.startswith("trace_mode"):
        kw["trace_mode"] = int(variant[-1])
    elif variant == "max_error8":
        max_error = 8
    elif variant == "small_arena":
        kw["arena_bytes"] = 1 << 20      # (a fixed arena of 1 MiB: a group of `small` does not fit it at once)
    al = wfagpu.DeviceAligner(0, **kw)
    try:
        passes = retried = 0
        for name in ef.SETS:
            g = sets[name]
            scores, cigars, ends, stats = _run_set(al, g, True, max_error or MAX_ERROR[name])
            _check_set(g, scores, cigars, ends, True)
            passes = max(passes, max(st.sub_batches for st in stats))
            retried += sum(st.pairs_retried for st in stats)
            if variant.startswith("min_tier"):
                t = int(variant[-1])
                assert all(sum(st.pairs_tier[:t]) == 0 for st in stats)
        if variant == "max_error8":
            assert retried > 200
        if variant == "small_arena":
            assert passes > 1
    finally:
        al.close()


def test_byte_compare_class(sets):
    """Pairs with N / IUPAC bytes run in the byte-compare kernels (WFA2 compares bytes as they are)."""
    g = sets["small"]
    only = {i for i, (p, t) in enumerate(g["pairs"]) if set(p + t) - set(b"ACGT")}
    assert len(only) >= 8
    al = wfagpu.DeviceAligner(0)
    try:
        for cigar in (False, True):
            scores, cigars, ends, stats = _run_set(al, g, cigar, MAX_ERROR["small"], only=only)
            _check_set(g, scores, cigars, ends, cigar, only=only)
            assert sum(st.pairs_raw for st in stats) == len(only)
    finally:
        al.close()


def test_big_batch(sets):
    """More than 8192 pairs in one call (where an end-to-end call would draw a sample for score budgets): small 21 times over in a
    seeded shuffle, all under one span."""
    g = sets[ef.ONE_SPAN_SET]
    order = list(range(len(g["pairs"]))) * 21
    random.Random(5).shuffle(order)
    assert len(order) >= 8192
    buf, meta = wfagpu.layout_pairs([g["pairs"][i] for i in order])
    al = wfagpu.DeviceAligner(0)
    try:
        batch = al.upload(buf, meta)
        want_s = g["scores"][order]
        s, _ = al.align(batch, ef.ONE_SPAN_PEN, max_error=600, compute_cigar=False, span=ef.ONE_SPAN)
        assert np.array_equal(s, want_s)
        s, c = al.align(batch, ef.ONE_SPAN_PEN, max_error=600, compute_cigar=True, span=ef.ONE_SPAN)
        assert np.array_equal(s, want_s)
        assert c == [g["cigars"][i] for i in order]
        assert al.stats().auto_budget == 0      # (no budgets from a sample under a span)
    finally:
        al.close()


def _launch(pairs, pen, cigar, max_error, batch_size, band=-1, band_width=0):
    lib = wfagpu.load()
    buf, meta = wfagpu.layout_pairs(pairs)
    n = len(pairs)
    res = C.POINTER(wfagpu.AlignmentResult)()
    assert lib.initialize_wfa_results(C.byref(res), n, 256 if cigar else 1)
    opt = wfagpu.Options(max_error=max_error, threads_per_block=band_width, num_workers=1, band=band, batch_size=batch_size,
                         num_alignments=n, penalties=wfagpu.Penalties(*pen), compute_cigar=cigar)
    fn = lib.launch_alignments if cigar else lib.launch_alignments_distance
    fn(buf.ctypes.data, buf.nbytes, meta.ctypes.data, res, opt, False)
    scores = np.array([res[i].error for i in range(n)], dtype=np.int64)
    cigars = [C.string_at(res[i].cigar.buffer).decode() for i in range(n)] if cigar else None
    lib.destroy_wfa_results(res, n)
    return scores, cigars


def test_configured_span_behind_the_launch_seam(sets, golden_dir):
    """wfagpu_amd_configure_span: launch_alignments and launch_alignments_distance on two device slots with a batch size that cuts
    the call; a band that is asked for gives the exact results; without a span the calls are end to end again."""
    g = sets[ef.ONE_SPAN_SET]
    pb, pe, tb, te = ef.ONE_SPAN
    e2e_pairs = wfagpu.read_seq_file(os.path.join(golden_dir, "seq1k.seq"))[:40]
    e2e_gold = -np.loadtxt(os.path.join(golden_dir, "seq1k.x2o3e1.scores"), dtype=np.int64)[:40]
    try:
        wfagpu.configure_launch(virtual_devices=2)
        wfagpu.configure_span(pattern_begin_free=pb, pattern_end_free=pe, text_begin_free=tb, text_end_free=te)
        s, c = _launch(g["pairs"], ef.ONE_SPAN_PEN, True, 600, 37)
        assert np.array_equal(s, g["scores"]) and c == g["cigars"]
        s, _ = _launch(g["pairs"], ef.ONE_SPAN_PEN, False, 600, 37)
        assert np.array_equal(s, g["scores"])
        s, c = _launch(g["pairs"], ef.ONE_SPAN_PEN, True, 600, 150, band=25, band_width=64)
        assert np.array_equal(s, g["scores"]) and c == g["cigars"]
        wfagpu.configure_span()
        s, _ = _launch(e2e_pairs, (2, 3, 1), True, 1000, 40)
        assert np.array_equal(s, e2e_gold)
    finally:
        wfagpu.configure_span()


def test_cli_ends_free(sets, tmp_path):
    """--ends-free with -x -c -o: the golden lines, and the -c verification (CIGAR priced without its free runs, score against the
    ends-free CPU program) finds nothing wrong."""
    g = sets[ef.ONE_SPAN_SET]
    seq = tmp_path / "nonempty.seq"      # (a .seq file carries no empty sequence)
    keep = [i for i, (p, t) in enumerate(g["pairs"]) if p and t]
    with open(seq, "wb") as f:
        for i in keep:
            f.write(b">" + g["pairs"][i][0] + b"\n<" + g["pairs"][i][1] + b"\n")
    out = tmp_path / "res.out"
    r = subprocess.run([CLI, "-i", str(seq), "--ends-free", ",".join(str(v) for v in ef.ONE_SPAN), "-g", "2,3,1", "-e", "600", "-x", "-c",
                        "-b", "150", "-o", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Incorrect=0" in r.stderr and all(tok == "Incorrect=0" for tok in r.stderr.split() if tok.startswith("Incorrect="))
    got = open(out).read().splitlines()
    assert got == [f"{-int(g['scores'][i])}\t{g['cigars'][i]}" for i in keep]


# ---- the sweep: eight penalty sets under five spans and tight budgets (endsfree_ref.SWEEP_PENS, SWEEP_SPANS) -----------------------
SWEEP_PATHS = ["as shipped", "min_tier1", "min_tier2", "min_tier3", "max_error8"]


@pytest.fixture(scope="module")
def sweep():
    return ef.read_golden(ef.SWEEP_SET)


def _factor(key):
    return math.gcd(*key[1])


@pytest.mark.parametrize("cigar", [False, True])
@pytest.mark.parametrize("path", SWEEP_PATHS)
def test_sweep_golden(sweep, cigar, path):
    """Every (span, penalties) group of the sweep as one call under a budget of its largest golden score plus 1 (max_error8: of 8) -- as
    shipped and forced through the wider tiers: WFA2's scores and CIGAR bytes."""
    g = sweep
    al = wfagpu.DeviceAligner(0, **({"min_tier": int(path[-1])} if path.startswith("min_tier") else {}))
    try:
        for key, idx in ef.groups(g).items():
            budget = 8 if path == "max_error8" else int(g["scores"][idx].max()) + 1
            scores, cigars, ends, (st,) = _run_set(al, g, cigar, budget, only=set(idx))
            _check_set(g, scores, cigars, ends, cigar, only=set(idx))
            if path.startswith("min_tier"):
                assert sum(st.pairs_tier[:int(path[-1])]) == 0, key
            if path == "max_error8":
                assert st.pairs_retried >= ef.sweep_over(g["scores"][idx], 8, _factor(key)), key
    finally:
        al.close()


def test_ring_depth_on_either_side_of_the_one_wave_limit(sweep):
    """plan_tier keeps an M ring of more than 64 rows (max(x, o + e) + 1: endsfree_ref.ring_depth) off the one-wave tier: as shipped,
    under budgets just above the golden scores, a penalty set whose ring has at most 64 rows has pairs on tier 0 and no call of one
    with a deeper ring has any -- and both give WFA2's bytes.  The rows are those of the penalties without their common factor:
    (2,62,2) runs as (1,31,1), 33 rows, (3,61,2) is the set with 64 and (2,63,2) has 66.  Counted per penalty set, over its five spans:
    the window of a span is wider by the free bases, and the all-free span of a 700-base pair is every diagonal there is, which no
    one-wave ring holds."""
    g = sweep
    al = wfagpu.DeviceAligner(0)
    try:
        tier0, depths = {}, {}
        for (span, pen), idx in ef.groups(g).items():
            scores, cigars, ends, (st,) = _run_set(al, g, True, int(g["scores"][idx].max()) + 1, only=set(idx))
            _check_set(g, scores, cigars, ends, True, only=set(idx))
            depths[pen] = ef.ring_depth(pen)
            tier0[pen] = tier0.get(pen, 0) + st.pairs_tier[0]
            assert depths[pen] <= 64 or st.pairs_tier[0] == 0, (span, pen, list(st.pairs_tier))
        assert set(tier0) == set(ef.SWEEP_PENS) and {64, 66} <= set(depths.values())
        for pen in ef.SWEEP_PENS:
            assert (tier0[pen] > 0) == (depths[pen] <= 64), (pen, depths[pen], tier0[pen])
    finally:
        al.close()


def test_score_budget_window_is_exact(sweep):
    """The counterpart of test_gpu_parity.py's test_score_budget_window_is_exact: the pairs of a (span, penalties) group that share a
    golden score run under a budget of exactly that score and of one less -- every pair comes back for a wider ring then --, and give
    WFA2's bytes both times.  At the score itself only the results are asserted: the ends-free window is a bound for the longest pair
    of the call (plan_tier), and a shorter pair whose own window is wider legitimately comes back as a window failure.  (6,9,3) runs as
    (2,3,1) and (2,62,2) as (1,31,1) with the budget divided by the factor, rounded down: score and score - 1 still fall on either
    side.  (The all-free span scores 0 everywhere and has no budget to run under.)"""
    g = sweep
    chosen = ef.sweep_budget_groups(list(zip(g["spans"], g["pens"])), g["scores"], _factor, seed=20261011)
    assert {k[1] for k, _, _ in chosen} == set(ef.SWEEP_PENS) and {k[0] for k, _, _ in chosen} == set(ef.SWEEP_SPANS[:4]) and len(chosen) <= 48
    al = wfagpu.DeviceAligner(0)
    try:
        for key, score, idx in chosen:
            for budget in (score, score - 1):
                scores, cigars, ends, (st,) = _run_set(al, g, True, budget, only=set(idx))
                _check_set(g, scores, cigars, ends, True, only=set(idx))
                if budget < score:
                    assert st.pairs_retried == len(idx), (key, score, budget, len(idx))
    finally:
        al.close()


def test_sweep_behind_the_launch_seam(sweep):
    """wfagpu_amd_configure_span with each span of the sweep under penalties that have a common factor and under a ring deeper than 64
    rows, through launch_alignments with a batch size that cuts the call: the golden bytes."""
    g = sweep
    groups = ef.groups(g)
    try:
        for pen in ((6, 9, 3), (2, 63, 2)):
            for span in ef.SWEEP_SPANS:
                idx = groups[(span, pen)]
                pb, pe, tb, te = span
                wfagpu.configure_span(pattern_begin_free=pb, pattern_end_free=pe, text_begin_free=tb, text_end_free=te)
                s, c = _launch([g["pairs"][i] for i in idx], pen, True, int(g["scores"][idx].max()) + 1, 3)
                assert np.array_equal(s, g["scores"][idx]) and c == [g["cigars"][i] for i in idx], (span, pen)
    finally:
        wfagpu.configure_span()
