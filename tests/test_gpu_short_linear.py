"""Tier 5 under the edit, indel and gap-linear metrics (short_kernel_lin.hip: several alignments per wavefront, the M ring in
registers) through the existing doors, against WFA2's scores and CIGAR bytes (tests/golden/linear.*, read through linear_ref).
A budget is in the metric's own units; it plans 8 lanes up to budget / g = 6, 16 up to 14, 32 up to 30."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import linear_ref as lr
import wfagpu

pytestmark = pytest.mark.gpu
LIN32 = ("linear", 3, 2)


def _run(al, g, idx, metric, cigar, max_error):
    """One call on the pairs idx of a golden set: WFA2's scores and bytes; -> the call's stats."""
    buf, meta = wfagpu.layout_pairs([g["pairs"][i] for i in idx])
    s, c = al.align(al.upload(buf, meta), None, max_error=max_error, compute_cigar=cigar, linear=metric)
    assert np.array_equal(s, g["scores"][idx]), (metric, max_error)
    if cigar:
        assert list(c) == [g["cigars"][i] for i in idx], (metric, max_error)
    return al.stats()


@pytest.mark.parametrize("lanes", [16, 32])
@pytest.mark.parametrize("no_fused_pack", [0, 1])
@pytest.mark.parametrize("cigar,off", [(False, ""), (True, ""), (False, "min_tier"), (True, "min_tier"), (True, "no_short_cigar")])
def test_ties_on_the_short_tier(lanes, cigar, no_fused_pack, off):
    """Every golden score of ties is within the budget: all pairs finish on tier 5, from ASCII and from packed words, with the golden
    bytes (the gap can sit anywhere in a repeat: the priority decides them); with the tier switched off, none and the same bytes."""
    g = lr.read_golden("ties")
    al = wfagpu.DeviceAligner(0, no_fused_pack=no_fused_pack, **({off: 1} if off else {}))
    try:
        for metric, idx in lr.groups(g).items():
            st = _run(al, g, idx, metric, cigar, (lanes - 2) * lr.pens_of(metric)[1])
            assert st.pairs_tier[5] == (0 if off else len(idx)), (metric, list(st.pairs_tier))
            assert off or (st.main_launch_tier == 5 and st.waves_per_simd_tier0 == lanes)
    finally:
        al.close()


@pytest.mark.parametrize("metric", [lr.EDIT, lr.INDEL, LIN32])
def test_budget_equal_to_the_score_and_one_step_less(metric):
    """The pairs of a metric that share a golden score under a budget of exactly that score: all finish on tier 5, none is retried;
    under score - g: none finishes in that launch, every pair is retried (under four times the budget: on tier 5 again where that
    still fits); the golden bytes both times.  Budgets up to 6 g run on 8 lanes."""
    g = lr.read_golden("ties")
    gap = lr.pens_of(metric)[1]
    idx_m = lr.groups(g)[metric]
    al = wfagpu.DeviceAligner(0)
    try:
        for score in sorted({int(g["scores"][i]) for i in idx_m if g["scores"][i] > gap}):
            idx = [i for i in idx_m if g["scores"][i] == score]
            st = _run(al, g, idx, metric, True, score)
            assert st.pairs_tier[5] == len(idx) and st.pairs_retried == 0, (score, list(st.pairs_tier))
            assert st.waves_per_simd_tier0 == (8 if score // gap <= 6 else 16)
            st = _run(al, g, idx, metric, True, score - gap)
            assert st.pairs_retried == len(idx), (score, list(st.pairs_tier))
    finally:
        al.close()


@pytest.mark.parametrize("cigar", [False, True])
def test_misses_and_the_byte_compare_class_in_one_call(cigar):
    """small_edit under max_error = 30: about half the pairs are unrelated and miss the budget, two hold an empty sequence, one is
    identical, thirteen hold N / IUPAC bytes.  Tier 5 finishes exactly the ACGT-only pairs whose golden score is within the budget."""
    g = lr.read_golden("small_edit")
    acgt = np.array([not (set(p + t) - set(b"ACGT")) for p, t in g["pairs"]])
    al = wfagpu.DeviceAligner(0)
    try:
        st = _run(al, g, list(range(len(acgt))), lr.EDIT, cigar, 30)
        assert int((g["scores"] <= 30).sum()) == 202
        assert st.pairs_tier[5] == int((acgt & (g["scores"] <= 30)).sum()), list(st.pairs_tier)
        assert st.pairs_raw == int((~acgt).sum()) == 13
    finally:
        al.close()


@pytest.mark.parametrize("metric", [lr.INDEL, ("linear", 4, 2), ("linear", 1, 3), ("linear", 5, 1)])
def test_small_under_the_other_metrics(metric):
    """No mismatch move, a common factor, x < g and x > 2 g, each at the largest budget that plans 32 lanes."""
    g = lr.read_golden("small")
    idx = lr.groups(g)[metric]
    budget = 30 * lr.pens_of(metric)[1]
    al = wfagpu.DeviceAligner(0)
    try:
        for cigar in (False, True):
            st = _run(al, g, idx, metric, cigar, budget)
            assert st.pairs_tier[5] > 0 or not (g["scores"][idx] <= budget).any(), list(st.pairs_tier)      # ((5,1): no score within 30)
    finally:
        al.close()


_FRESH_PROCESS = r"""
import wfagpu
lib = wfagpu.load()
buf, meta = wfagpu.generate_pairs(64, 150, 0.02, seed=11)
al = wfagpu.DeviceAligner(0)
assert lib.wfagpu_amd_prime(al.ctx) == 0
batch = al.upload(buf, meta)
al.align(batch, (2, 3, 1), max_error=14, compute_cigar=True)
print("affine", al.stats().pairs_tier[5] > 0, lib.wfagpu_amd_debug_code_objects() & 128)
al.align(batch, None, max_error=100, compute_cigar=True, linear=("edit",))
print("wide", lib.wfagpu_amd_debug_code_objects() & 128)
al.align(batch, None, max_error=12, compute_cigar=True, linear=("edit",))
print("short", lib.wfagpu_amd_debug_code_objects() & 128)
al.close()
"""


def test_only_a_metric_call_that_fits_loads_the_code_object():
    """A fresh process: prime with nothing configured, a gap-affine call on tier 5 and an edit call whose budget is too wide leave bit 7
    of wfagpu_amd_debug_code_objects clear; an edit call under max_error = 12 sets it."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(os.path.abspath(wfagpu.__file__)), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", _FRESH_PROCESS], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["affine", "True", "0", "wide", "0", "short", "128"], r.stdout


@pytest.mark.parametrize("cigar", [False, True])
def test_a_configured_metric_behind_the_launch_seam(cigar):
    """wfagpu_amd_configure_linear(edit), then launch_alignments_distance / launch_alignments with a batch size that cuts the call."""
    g = lr.read_golden("ties")
    idx = lr.groups(g)[lr.EDIT]
    pairs = [g["pairs"][i] for i in idx]
    lib = wfagpu.load()
    buf, meta = wfagpu.layout_pairs(pairs)
    res = C.POINTER(wfagpu.AlignmentResult)()
    assert lib.initialize_wfa_results(C.byref(res), len(pairs), 256 if cigar else 1)
    opt = wfagpu.Options(max_error=14, threads_per_block=0, num_workers=1, band=-1, batch_size=4, num_alignments=len(pairs),
                         penalties=wfagpu.Penalties(2, 3, 1), compute_cigar=cigar)
    try:
        wfagpu.configure_linear(lr.EDIT)
        (lib.launch_alignments if cigar else lib.launch_alignments_distance)(buf.ctypes.data, buf.nbytes, meta.ctypes.data, res, opt, False)
        assert [res[i].error for i in range(len(pairs))] == [int(g["scores"][i]) for i in idx]
        if cigar:
            assert [C.string_at(res[i].cigar.buffer).decode() for i in range(len(pairs))] == [g["cigars"][i] for i in idx]
    finally:
        wfagpu.configure_linear()
        lib.destroy_wfa_results(res, len(pairs))
