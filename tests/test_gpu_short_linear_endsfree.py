"""Tier 5 for the edit, indel and gap-linear metrics under an ends-free span (short_kernel_linef.hip: groups of 16, 32 or 64 lanes, the
M ring in registers) through the existing doors, against linear_endsfree_ref.wfa_linear_endsfree_model -- score, CIGAR bytes, (k0, k1);
the CPU suite pins the model to WFA2 -- and dp_linear_endsfree_score.  Every pair is a literal shape built here.

plan_tier's bound is S / g + 1 diagonals plus the four free-base counts, each clamped to the batch's longest sequence; the smallest
of 16 / 32 / 64 lanes with one lane to spare takes the call (_lanes below restates it).  Two things follow for the cases:
  * a text lead of up to 47 bases under (0, 0, 50, 50) is bounded by 2 + 1 + 100 diagonals: no group holds that, whatever the pairs'
    own windows are.  The seam cases therefore free only the 6-base tail at the text's end -- (0, 0, 50, 6): 59 diagonals, 64 lanes;
    (0, 0, 20, 6): 29, 32 lanes -- and `seams_50_50` runs the wider span as it stands: the same bytes, on the one-wave tier.
  * a pair's own window is never wider than the bound, and the bound leaves a lane to spare: own windows of L and L + 1 diagonals at a
    planned L do not exist, a BAND failure cannot be had from this tier under the default rule.  No case for it."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import endsfree_ref as er
import linear_endsfree_ref as ler
import linear_ref as lr
import wfagpu

pytestmark = pytest.mark.gpu
INT32_MIN = -(2**31)
LIN32, LIN42 = ("linear", 3, 2), ("linear", 4, 2)
METRICS = (lr.EDIT, lr.INDEL, LIN32, LIN42)
LEADS = (0, 1, 14, 15, 16, 17, 31, 32, 33, 47)


def _sub(s, i):
    return s[:i] + bytes([b"ACGT"[(b"ACGT".index(s[i]) + 1) % 4]]) + s[i + 1:]


def _cases():
    """name -> (metric, span, max_error, lanes or None, pairs)"""
    rng = er.Rng(20261126)
    read = rng.seq(20)
    hit = _sub(read, 9)
    seams = [(read, rng.seq(lead) + hit + rng.seq(6)) for lead in LEADS]
    out = {"seams_64": (lr.EDIT, (0, 0, 50, 6), 2, 64, seams), "seams_32": (lr.EDIT, (0, 0, 20, 6), 2, 32, seams[:6]),
           "seams_16": (lr.EDIT, (0, 0, 5, 5), 2, 16, [(read, rng.seq(lead) + hit + rng.seq(5)) for lead in (0, 1, 4, 5)]),
           "seams_50_50": (lr.EDIT, (0, 0, 50, 50), 2, None, seams),
           "with_n": (lr.EDIT, (0, 0, 50, 6), 2, 64, seams[:3] + [(read[:5] + b"N" + read[6:], seams[3][1])])}
    # each kind of span: the pattern sticks out in front / behind, the text behind, all four; one substitution and one deleted base
    core = rng.seq(24)
    dmg = _sub(core, 6)[:15] + _sub(core, 6)[16:]
    kinds = {(6, 0, 0, 0): (rng.seq(4) + core, dmg), (0, 6, 0, 0): (core + rng.seq(4), dmg), (0, 0, 0, 7): (core, dmg + rng.seq(5)),
             (7, 3, 5, 9): (rng.seq(3) + core + rng.seq(2), rng.seq(4) + dmg + rng.seq(6))}
    for metric in METRICS:
        for span, pair in kinds.items():
            out["span_%s_%s" % ("_".join(map(str, metric)), "_".join(map(str, span)))] = (metric, span, 12, None, [pair, (pair[0], _sub(pair[1], 2))])
    # either side of the packed-word seam and of the 32-base extend round trip
    reads = [rng.seq(n) for n in (15, 16, 17, 31, 32, 33, 65)]
    out["lengths"] = (lr.EDIT, (0, 0, 4, 4), 4, 16, [(r, rng.seq(3) + _sub(r, len(r) // 2) + rng.seq(3)) for r in reads])
    out["empties"] = (lr.EDIT, (2, 2, 3, 3), 12, 32, [(b"", rng.seq(10)), (rng.seq(10), b"")])
    unit = rng.seq(8)
    out["tied_ends"] = (lr.EDIT, (0, 0, er.INT_MAX, er.INT_MAX), 2, 64, [(unit, unit * 3), (_sub(unit, 3), unit * 3)])
    return out


CASES = _cases()
_MODEL = {}


def _lanes(metric, span, max_error, pairs):
    """plan_tier's rule (wfa_host.hip) -> lanes, or None where the bound does not fit a group."""
    x, g = lr.pens_of(metric)
    f = g if x is None else math.gcd(x, g)
    m = max(max(len(p), len(t)) for p, t in pairs)
    width = min(2 * m + 1, max(1, max_error // f) // (g // f) + 1 + sum(min(v, m) for v in span))
    return next((l for l in (16, 32, 64) if width + 1 <= l), None)


def _own_window(p, t, metric, span, budget):
    """DESIGN section 4.10, "Window" -> diagonals of the pair's own window under the budget"""
    kend, gb = len(t) - len(p), budget // lr.pens_of(metric)[1]
    pb, pe, tb, te = er.clamp_span(span, len(p), len(t))
    a_hi, a_lo = gb + tb + kend + pe, gb + pb + te - kend
    whi = max(tb, kend + pe, min(len(t), a_hi // 2) if a_hi >= 0 else -len(p))
    wlo = min(-pb, kend - te, -min(len(p), a_lo // 2) if a_lo >= 0 else len(t))
    return min(whi, len(t)) - max(wlo, -len(p)) + 1


def _model(name, max_error=None):
    """The case's reference, computed once: [(score, cigar, (k0, k1))]; budget and window asserted here, before any GPU call."""
    metric, span, me, lanes, pairs = CASES[name]
    me = me if max_error is None else max_error
    if name not in _MODEL:
        _MODEL[name] = [ler.wfa_linear_endsfree_model(p, t, metric, span) for p, t in pairs]
        x, g = lr.pens_of(metric)
        assert [r[0] for r in _MODEL[name]] == [ler.dp_linear_endsfree_score(p, t, x, g, span) for p, t in pairs], name
    planned = _lanes(metric, span, me, pairs)
    assert lanes in (None, planned) and (planned is not None or name == "seams_50_50"), (name, planned)
    if planned:
        assert all(_own_window(p, t, metric, span, me) <= planned for p, t in pairs), name
    return _MODEL[name], planned


def _call(al, name, cigar, max_error=None):
    """One call on the case's pairs: the model's scores, end diagonals and (with CIGARs) bytes and start diagonals -> stats, lanes."""
    metric, span, me, _, pairs = CASES[name]
    ref, planned = _model(name, max_error)
    buf, meta = wfagpu.layout_pairs(pairs)
    s, c, e = al.align(al.upload(buf, meta), None, max_error=me if max_error is None else max_error, compute_cigar=cigar, linear=metric,
                       span=span, fetch_ends=True)
    assert list(s) == [r[0] for r in ref], name
    assert list(e[:, 1]) == [r[2][1] for r in ref], name
    if cigar:
        assert list(c) == [r[1] for r in ref] and list(e[:, 0]) == [r[2][0] for r in ref], name
        for (p, t), cg, sc, en in zip(pairs, c, s, e):
            assert ler.check_cigar_linear_span(p, t, cg, metric, span, ends=(int(en[0]), int(en[1]))) == (True, sc), name
    else:
        assert (e[:, 0] == INT32_MIN).all(), name
    return al.stats(), planned


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("off", ["", "min_tier", "no_short_cigar"])
def test_cases_on_the_short_tier(name, off):
    """Score-only and with CIGARs, from ASCII and from packed words: every ACGT pair whose call the rule plans finishes on tier 5 on
    the planned lanes (the pair with an N in the byte-compare class); with the tier switched off none does; the model's bytes always."""
    ref, planned = _model(name)
    assert all(r[0] <= CASES[name][2] for r in ref), name
    raw = sum(1 for p, t in CASES[name][4] if set(p + t) - set(b"ACGT"))
    assert raw == (1 if name == "with_n" else 0)
    for no_fused_pack in (0, 1):
        al = wfagpu.DeviceAligner(0, no_fused_pack=no_fused_pack, **({off: 1} if off else {}))
        try:
            for cigar in (False, True):
                st, _ = _call(al, name, cigar)
                on = planned and not (off == "min_tier" or (off and cigar))
                assert st.pairs_tier[5] == (len(ref) - raw if on else 0) and st.pairs_raw == raw, (name, cigar, list(st.pairs_tier))
                # (main_launch_tier is the call's longest launch and the byte-compare class launches last: both are that class's in with_n)
                assert not on or raw or (st.main_launch_tier == 5 and st.waves_per_simd_tier0 == planned), (name, st.waves_per_simd_tier0)
        finally:
            al.close()


@pytest.mark.parametrize("metric", METRICS)
def test_budget_equal_to_the_score_and_one_gap_less(metric):
    """The window is exact: the (7, 3, 5, 9) pairs of a metric under a budget of exactly their score all finish on tier 5 and none is
    retried; under that budget minus g every pair is "not within the budget", comes back and gives the same bytes."""
    name = "span_%s_7_3_5_9" % "_".join(map(str, metric))
    scores = {r[0] for r in _model(name)[0]}
    assert len(scores) == 1 and min(scores) >= 2 * lr.pens_of(metric)[1]
    al = wfagpu.DeviceAligner(0)
    try:
        st, planned = _call(al, name, True, max_error=min(scores))
        assert st.pairs_tier[5] == 2 and st.pairs_retried == 0 and st.waves_per_simd_tier0 == planned, list(st.pairs_tier)
        st, _ = _call(al, name, True, max_error=min(scores) - lr.pens_of(metric)[1])
        assert st.pairs_retried == 2 and st.main_launch_tier == 5, list(st.pairs_tier)
    finally:
        al.close()


def test_the_hook_forces_wider_groups():
    """tuning.waves_per_simd = 32 / 64: at least that many lanes for a call that plans 16."""
    for lanes in (32, 64):
        al = wfagpu.DeviceAligner(0, waves_per_simd=lanes)
        try:
            st, _ = _call(al, "lengths", True)
            assert st.pairs_tier[5] == 7 and st.waves_per_simd_tier0 == lanes
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
al.align(batch, None, max_error=12, compute_cigar=True, linear=("edit",))
print("end-to-end", al.stats().pairs_tier[5] > 0, lib.wfagpu_amd_debug_code_objects() & 256)
al.align(batch, None, max_error=100, compute_cigar=True, linear=("edit",), span=(0, 0, 8, 8))
print("wide", al.stats().pairs_tier[5], lib.wfagpu_amd_debug_code_objects() & 256)
al.align(batch, None, max_error=12, compute_cigar=True, linear=("edit",), span=(0, 0, 8, 8))
print("short", al.stats().pairs_tier[5] > 0, lib.wfagpu_amd_debug_code_objects() & 256)
al.close()
"""


def test_only_a_span_call_that_fits_loads_the_code_object():
    """A fresh process: prime with nothing configured, a gap-affine call, an end-to-end edit call on tier 5 and a span call under
    max_error = 100 leave bit 8 of wfagpu_amd_debug_code_objects clear; a span call under max_error = 12 sets it."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(os.path.abspath(wfagpu.__file__)), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", _FRESH_PROCESS], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["end-to-end", "True", "0", "wide", "0", "0", "short", "True", "256"], r.stdout


@pytest.mark.parametrize("cigar", [False, True])
def test_a_metric_configured_with_a_span_behind_the_launch_seam(cigar):
    """wfagpu_amd_configure_linear_span(edit, (0, 0, 50, 6)), then launch_alignments_distance / launch_alignments with a batch size that
    cuts the ten seam pairs into calls of four."""
    metric, span, max_error, _, pairs = CASES["seams_64"]
    ref, _ = _model("seams_64")
    lib = wfagpu.load()
    buf, meta = wfagpu.layout_pairs(pairs)
    res = C.POINTER(wfagpu.AlignmentResult)()
    assert lib.initialize_wfa_results(C.byref(res), len(pairs), 256 if cigar else 1)
    opt = wfagpu.Options(max_error=max_error, threads_per_block=0, num_workers=1, band=-1, batch_size=4, num_alignments=len(pairs),
                         penalties=wfagpu.Penalties(2, 3, 1), compute_cigar=cigar)
    try:
        wfagpu.configure_linear(metric, span=span)
        (lib.launch_alignments if cigar else lib.launch_alignments_distance)(buf.ctypes.data, buf.nbytes, meta.ctypes.data, res, opt, False)
        assert [res[i].error for i in range(len(pairs))] == [r[0] for r in ref]
        if cigar:
            assert [C.string_at(res[i].cigar.buffer).decode() for i in range(len(pairs))] == [r[1] for r in ref]
    finally:
        wfagpu.configure_linear()
        lib.destroy_wfa_results(res, len(pairs))
