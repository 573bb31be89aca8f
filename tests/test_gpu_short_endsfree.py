"""Tier 5 for gap-affine alignment under an ends-free span (short_kernel_ef*.hip: groups of 16, 32 or 64 lanes, M, I and D rings in
registers) through the existing doors, against WFA2's own scores and CIGAR bytes: tests/golden/endsfree.short.alg, one "-score<TAB>CIGAR"
line per pair of CASES in sorted order of the names (endsfree_ref.wfa2_endsfree wrote it; test_fixture_is_wfa2 pins it).  Every pair is a
literal shape built here, and the lanes plan_tier picks -- the smallest of 16 / 32 / 64 with (max_error - o) / e + 1 plus the four
clamped free-base counts plus one -- stand in each case as a literal.  (k0, k1) are checked through the fixture's CIGAR: check_cigar
prices it with exactly the free bases the two diagonals say, and that price must be the fixture's score."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import endsfree_ref as er
import oracle_lib
import wfagpu

INT32_MIN = -(2**31)
LEADS = (0, 1, 14, 15, 16, 17, 31, 32, 33, 47)


def _sub(s, i):
    return s[:i] + bytes([b"ACGT"[(b"ACGT".index(s[i]) + 1) % 4]]) + s[i + 1:]


def _cases():
    """name -> (penalties, span, max_error, lanes, pairs)"""
    rng = er.Rng(20261127)
    read = rng.seq(20)
    hit = _sub(read, 9)
    # start and end diagonals at lane 0, at the last lane and on either side of every DPP row boundary
    seams = [(read, rng.seq(lead) + hit + rng.seq(6)) for lead in LEADS]
    out = {"seams_64": ((2, 3, 1), (0, 0, 50, 6), 2, 64, seams), "seams_32": ((2, 3, 1), (0, 0, 20, 6), 2, 32, seams[2:6]),
           "seams_16": ((2, 3, 1), (0, 0, 5, 5), 2, 16, [(read, rng.seq(lead) + hit + rng.seq(5)) for lead in (0, 1, 4, 5)]),
           "with_n": ((2, 3, 1), (0, 0, 50, 6), 2, 64, seams[:1] + [(read[:9] + b"N" + read[10:], seams[3][1])])}
    # I and D rings: a planted insertion / deletion of 1, 2 and 5 bases mid-read, and one that continues a free run at the sequence's end
    # (the trailing run of the CIGAR is then partly free, partly paid)
    core, lead = rng.seq(24), rng.seq(4)
    gaps = [(core, lead + core[:12] + rng.seq(n) + core[12:] + rng.seq(3)) for n in (1, 5)] + [(core, lead + core + rng.seq(5 + 2))]
    gaps += [(core, lead + core[:12] + core[12 + 2:] + rng.seq(3))] + [(core + rng.seq(4 + n), lead + core) for n in (1, 5)]
    for pen, max_error, lanes in (((2, 3, 1), 8, 32), ((5, 3, 2), 60, 64), ((7, 2, 3), 20, 32), ((3, 1, 4), 100, 64), ((4, 6, 2), 16, 32)):
        out["gaps_%d_%d_%d" % pen] = (pen, (3, 4, 6, 5), max_error, lanes, gaps)
    # each kind of span: the pattern sticks out in front / behind, the text behind, all four; one substitution and one deleted base
    dmg = _sub(core, 6)[:15] + _sub(core, 6)[16:]
    kinds = {(6, 0, 0, 0): (rng.seq(4) + core, dmg), (0, 6, 0, 0): (core + rng.seq(4), dmg), (0, 0, 0, 7): (core, dmg + rng.seq(5)),
             (7, 3, 5, 9): (rng.seq(3) + core, dmg + rng.seq(6))}
    for span, pair in kinds.items():
        # (a second substitution: in the aligned part, or -- all four: the budget case wants one score -- in the free tail of the text)
        other = (pair[0], _sub(pair[1], len(pair[1]) - 1 if span == (7, 3, 5, 9) else 2))
        out["span_" + "_".join(map(str, span))] = ((5, 3, 2), span, 16, 32 if span == (7, 3, 5, 9) else 16, [pair, other])
    # either side of the packed-word seam and of the 32-base extend round trip
    reads = [rng.seq(n) for n in (15, 16, 17, 31, 32, 33, 65)]
    out["lengths"] = ((2, 3, 1), (0, 0, 4, 4), 4, 16, [(r, rng.seq(3) + _sub(r, len(r) // 2) + rng.seq(3)) for r in reads])
    out["empties"] = ((2, 3, 1), (2, 2, 3, 3), 12, 32, [(b"", rng.seq(10)), (rng.seq(10), b"")])
    unit = rng.seq(8)      # (several end diagonals at one score: the lowest wins)
    out["tied_ends"] = ((2, 3, 1), (0, 0, er.INT_MAX, er.INT_MAX), 2, 64, [(unit, unit * 3), (_sub(unit, 3), unit * 3)])
    return out


CASES = _cases()


_LINES = iter(open(os.path.join(er.GOLDEN, "endsfree.short.alg")).read().splitlines())
GOLD = {name: [(-int(s), c) for s, c in (next(_LINES).split("\t") for _ in CASES[name][4])] for name in sorted(CASES)}
assert next(_LINES, None) is None


def test_fixture_is_wfa2():
    """The fixture against the plain dynamic program and check_cigar, and -- where the reference library is built -- against WFA2 live."""
    for name, (pen, span, max_error, _, pairs) in CASES.items():
        for (p, t), (score, cigar) in zip(pairs, GOLD[name]):
            assert score == er.dp_endsfree_score(p, t, pen, span) and score <= max_error, name
            assert er.check_cigar(p, t, cigar, pen, span) == (True, score), (name, cigar)
        if oracle_lib.have_ref():
            s, c = er.wfa2_endsfree(pairs, [span] * len(pairs), [pen] * len(pairs))
            assert (list(s), c) == ([g[0] for g in GOLD[name]], [g[1] for g in GOLD[name]]), name


def _call(al, name, cigar, max_error=None):
    """One call on the case's pairs: the fixture's scores and (with CIGARs) bytes, diagonals that price the CIGAR at the score -> stats"""
    pen, span, me, _, pairs = CASES[name]
    buf, meta = wfagpu.layout_pairs(pairs)
    s, c, e = al.align(al.upload(buf, meta), pen, max_error=me if max_error is None else max_error, compute_cigar=cigar, span=span, fetch_ends=True)
    assert list(s) == [g[0] for g in GOLD[name]], name
    for i, ((p, t), (score, want)) in enumerate(zip(pairs, GOLD[name])):
        pb, pe, tb, te = er.clamp_span(span, len(p), len(t))
        assert len(t) - len(p) - te <= e[i][1] <= len(t) - len(p) + pe, (name, i)
        if cigar:
            assert c[i] == want, (name, i)
            assert er.check_cigar(p, t, want, pen, span, ends=(int(e[i][0]), int(e[i][1]))) == (True, score), (name, i, list(e[i]))
        else:
            assert e[i][0] == INT32_MIN, (name, i)
    return al.stats()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("off", ["", "min_tier"])
def test_cases_on_the_short_tier(name, off):
    """Score-only and with CIGARs, from ASCII and from packed words: every ACGT pair finishes on tier 5 on the planned lanes (the pair with
    an N in the byte-compare class); with min_tier = 1 none does; the fixture's bytes always."""
    n, raw = len(CASES[name][4]), 1 if name == "with_n" else 0
    for no_fused_pack in (0, 1):
        al = wfagpu.DeviceAligner(0, no_fused_pack=no_fused_pack, **({off: 1} if off else {}))
        try:
            for cigar in (False, True):
                st = _call(al, name, cigar)
                assert st.pairs_tier[5] == (0 if off else n - raw) and st.pairs_raw == raw, (name, cigar, list(st.pairs_tier))
                # (main_launch_tier is the call's longest launch; the byte-compare class launches last)
                assert off or raw or (st.main_launch_tier == 5 and st.waves_per_simd_tier0 == CASES[name][3]), (name, st.waves_per_simd_tier0)
        finally:
            al.close()


@pytest.mark.gpu
def test_budget_equal_to_the_score_and_one_less():
    """The window is exact: the (7, 3, 5, 9) pairs under a budget of exactly their score finish on tier 5, none retried; under one
    less every pair is "not within the budget", comes back and gives the same bytes."""
    scores = {g[0] for g in GOLD["span_7_3_5_9"]}
    assert len(scores) == 1
    al = wfagpu.DeviceAligner(0)
    try:
        st = _call(al, "span_7_3_5_9", True, max_error=min(scores))
        assert st.pairs_tier[5] == 2 and st.pairs_retried == 0 and st.waves_per_simd_tier0 == 32, list(st.pairs_tier)
        st = _call(al, "span_7_3_5_9", True, max_error=min(scores) - 1)
        assert st.pairs_retried == 2, list(st.pairs_tier)
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
al.align(batch, None, max_error=12, compute_cigar=True, linear=("edit",), span=(0, 0, 8, 8))
print("others", al.stats().pairs_tier[5] > 0, lib.wfagpu_amd_debug_code_objects() & 512)
al.align(batch, (2, 3, 1), max_error=100, compute_cigar=True, span=(0, 0, 8, 8))
print("wide", al.stats().pairs_tier[5], lib.wfagpu_amd_debug_code_objects() & 512)
al.align(batch, (2, 3, 1), max_error=14, compute_cigar=True, span=(0, 0, 8, 8))
print("short", al.stats().pairs_tier[5] > 0, lib.wfagpu_amd_debug_code_objects() & 512)
al.close()
"""


@pytest.mark.gpu
def test_only_a_gap_affine_span_call_that_fits_loads_the_code_object():
    """A fresh process: prime with nothing configured, an end-to-end gap-affine call and an edit-with-span call on tier 5, and a gap-affine
    span call under max_error = 100 leave bit 9 of wfagpu_amd_debug_code_objects clear; the span call under max_error = 14 sets it."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(os.path.abspath(wfagpu.__file__)), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", _FRESH_PROCESS], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["others", "True", "0", "wide", "0", "0", "short", "True", "512"], r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("cigar", [False, True])
def test_a_configured_span_behind_the_launch_seam(cigar):
    """wfagpu_amd_configure_span((0, 0, 50, 6)), then launch_alignments_distance / launch_alignments with a batch size that cuts the ten
    seam pairs into calls of four."""
    pen, span, max_error, _, pairs = CASES["seams_64"]
    lib = wfagpu.load()
    buf, meta = wfagpu.layout_pairs(pairs)
    res = C.POINTER(wfagpu.AlignmentResult)()
    assert lib.initialize_wfa_results(C.byref(res), len(pairs), 256 if cigar else 1)
    opt = wfagpu.Options(max_error=max_error, threads_per_block=0, num_workers=1, band=-1, batch_size=4, num_alignments=len(pairs),
                         penalties=wfagpu.Penalties(*pen), compute_cigar=cigar)
    try:
        wfagpu.configure_span(pattern_begin_free=span[0], pattern_end_free=span[1], text_begin_free=span[2], text_end_free=span[3])
        (lib.launch_alignments if cigar else lib.launch_alignments_distance)(buf.ctypes.data, buf.nbytes, meta.ctypes.data, res, opt, False)
        assert [res[i].error for i in range(len(pairs))] == [g[0] for g in GOLD["seams_64"]]
        if cigar:
            assert [C.string_at(res[i].cigar.buffer).decode() for i in range(len(pairs))] == [g[1] for g in GOLD["seams_64"]]
    finally:
        wfagpu.configure_span()
        lib.destroy_wfa_results(res, len(pairs))
