"""Ends-free alignment without a GPU: the golden files against an independent dynamic program and (where the reference is
compiled in place) against WFA2 run live; the CIGAR checker; the host-side pieces -- wfagpu_amd_configure_span, the -c
verification under a span, the command line's usage errors."""
import ctypes as C
import hashlib
import math
import os
import subprocess

import numpy as np
import pytest

import endsfree_ref as ef
import oracle_lib
import wfagpu

PKG = os.path.dirname(wfagpu.LIB_PATH)
CLI = os.path.join(PKG, "bin", "wfa.affine.gpu")
ALL_SETS = ef.SETS + (ef.ONE_SPAN_SET,)
PAIRS_SHA1 = "9d4f4ef6593fc492d8ae20f3d05d1b5122989528"      # of the pairs of small, wide and ties as make_set builds them


@pytest.fixture(scope="module")
def sets():
    return {name: ef.read_golden(name) for name in ALL_SETS + (ef.SWEEP_SET,)}


def test_golden_sets_have_the_shapes_they_are_for(sets):
    small, wide, ties = sets["small"], sets["wide"], sets["ties"]
    assert len(small["pairs"]) == 400 and len(wide["pairs"]) == 48 and len(ties["pairs"]) == 32
    assert any(len(p) == 0 for p, _ in small["pairs"]) and any(len(t) == 0 for _, t in small["pairs"])
    assert max(max(len(p), len(t)) for p, t in small["pairs"]) <= 300
    assert sum(1 for p, t in small["pairs"] if set(p + t) - set(b"ACGT")) >= 8
    assert len(set(small["spans"])) == 9 and len(set(small["pens"])) == 4 and (0, 0, 0, 0) in small["spans"]
    assert sorted({sp[0] + sp[2] + 1 for sp in wide["spans"]}) == [63, 64, 65, 129, 257, 1025]
    assert all(1100 <= max(len(p), len(t)) <= 1300 for p, t in wide["pairs"])
    assert sum(os.path.getsize(ef.golden_path(name)) for name in ALL_SETS) < (1 << 20)
    # (the pairs are rebuilt, not stored: the recipe must give the same bytes everywhere)
    digest = hashlib.sha1(b"".join(p + b"|" + t + b"\n" for name in ef.SETS for p, t in sets[name]["pairs"])).hexdigest()
    assert digest == PAIRS_SHA1


def test_the_sweep_has_the_shape_it_is_for(sets):
    """8 penalty sets of 20 short pairs each, four under each of the five spans, and 5 long pairs -- one per span -- under M rings of 33 and
    66 rows; every penalty set has its byte-compare pair and its empty side; a deep ring gets short pairs (endsfree_ref.sweep_top)."""
    g = sets[ef.SWEEP_SET]
    groups = ef.groups(g)
    assert len(g["pairs"]) == 8 * 20 + 2 * 5 and len(ef.SWEEP_PENS) == 8 and len(ef.SWEEP_SPANS) == 5
    assert set(groups) == {(span, pen) for span in ef.SWEEP_SPANS for pen in ef.SWEEP_PENS}
    assert (0, 0, 0, 0) in ef.SWEEP_SPANS and (ef.INT_MAX,) * 4 in ef.SWEEP_SPANS
    assert sorted(ef.ring_depth(pen) for pen in ef.SWEEP_PENS)[-4:] == [33, 41, 64, 66] and sum(1 for pen in ef.SWEEP_PENS if math.gcd(*pen) > 1) == 2
    assert [ef.ring_depth(pen) for pen in ef.SWEEP_LONG_PENS] == [33, 66]
    for pen in ef.SWEEP_PENS:
        idx = [i for i, q in enumerate(g["pens"]) if q == pen]
        short = [g["pairs"][i] for i in idx[:20]]
        assert len(idx) == (25 if pen in ef.SWEEP_LONG_PENS else 20)
        assert all(600 <= len(p) <= 800 and 600 <= len(t) <= 800 for p, t in (g["pairs"][i] for i in idx[20:]))
        assert sum(1 for p, t in short if set(p + t) - set(b"ACGT")) == 1 and sum(1 for p, t in short if not p or not t) == 1
        assert max(max(len(p), len(t)) for p, t in short) <= (48 if ef.ring_depth(pen) >= 60 else 160)
    assert any(not p for p, _ in g["pairs"]) and any(not t for _, t in g["pairs"])
    assert os.path.getsize(ef.golden_path(ef.SWEEP_SET)) < (64 << 10)


@pytest.mark.parametrize("name", ALL_SETS + (ef.SWEEP_SET,))
def test_golden_scores_equal_the_dynamic_program(sets, name):
    g = sets[name]
    for i, ((p, t), span, pen) in enumerate(zip(g["pairs"], g["spans"], g["pens"])):
        assert ef.dp_endsfree_score(p, t, pen, span) == g["scores"][i], (name, i, span, pen)


@pytest.mark.parametrize("name", ALL_SETS + (ef.SWEEP_SET,))
def test_golden_cigars_are_valid_and_cost_their_score(sets, name):
    g = sets[name]
    for i, ((p, t), span, pen) in enumerate(zip(g["pairs"], g["spans"], g["pens"])):
        ok, cost = ef.check_cigar(p, t, g["cigars"][i], pen, span)
        assert ok and cost == g["scores"][i], (name, i, span, pen, g["cigars"][i])


def test_cigar_checker_refuses_what_is_wrong():
    p, t, pen = b"ACGTACGT", b"TTACGAACGTGG", (2, 3, 1)
    assert ef.check_cigar(p, t, "2I3M1X4M2I", pen, (0, 0, 2, 2)) == (True, 2)
    assert ef.check_cigar(p, t, "2I3M1X4M2I", pen, (0, 0, 1, 2)) == (True, 2 + 3 + 1)      # one of the leading bases is paid for
    assert ef.check_cigar(p, t, "2I3M1X4M2I", pen, (0, 0, 0, 0)) == (True, 2 + 2 * (3 + 2))
    assert ef.check_cigar(p, t, "2I3M1X4M2I", pen, (0, 0, 2, 2), ends=(2, 2)) == (True, 2)
    assert not ef.check_cigar(p, t, "2I3M1X4M2I", pen, (0, 0, 2, 2), ends=(3, 2))[0]      # start diagonal outside the span
    assert not ef.check_cigar(p, t, "2I4M4M2I", pen, (0, 0, 2, 2))[0]                      # M on a mismatch, equal neighbours
    assert not ef.check_cigar(p, t, "2I3M1X4M1I", pen, (0, 0, 2, 2))[0]                    # does not cover the text


@pytest.mark.skipif(not oracle_lib.have_ref(), reason="the reference's WFA2 is not compiled in place here")
@pytest.mark.parametrize("name", ALL_SETS + (ef.SWEEP_SET,))
def test_wfa2_run_live_equals_the_golden_files(sets, name):
    g = sets[name]
    for mode in (0, 1):
        scores, cigars = ef.wfa2_endsfree(g["pairs"], g["spans"], g["pens"], memory_mode=mode)
        assert np.array_equal(scores, g["scores"]) and cigars == g["cigars"], (name, mode)


@pytest.mark.parametrize("args", [["--ends-free", "1,2"], ["--ends-free", "1,-2,0,0"], ["--ends-free", "0,0,5,5", "-B", "10"],
                                  ["--ends-free", "0,0,5,5x"]])
def test_cli_usage_errors_come_before_any_device_work(args, golden_dir):
    seq = os.path.join(golden_dir, "seq1k.seq")
    r = subprocess.run([CLI, "-i", seq] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "--ends-free" in r.stderr and "ERROR" in r.stderr
    assert "HIP device" not in r.stderr and "Reading sequences" not in r.stdout + r.stderr


def test_configure_span_rejects_negative_members_and_accepts_null():
    lib = wfagpu.load()
    assert "wfagpu_amd_align_device_span" in wfagpu.ABI_SYMBOLS and hasattr(lib, "wfagpu_amd_align_device_span")
    for bad in ((-1, 0, 0, 0), (0, -5, 0, 0), (0, 0, -1, 0), (0, 0, 0, -2**31)):
        assert lib.wfagpu_amd_configure_span(C.byref(wfagpu.Span(*bad))) == -1
    assert lib.wfagpu_amd_configure_span(C.byref(wfagpu.Span(0, 0, 2**31 - 1, 7))) == 0
    assert lib.wfagpu_amd_configure_span(None) == 0
    with pytest.raises(ValueError):
        wfagpu.configure_span(text_end_free=-3)
    wfagpu.configure_span(text_end_free=3)
    wfagpu.configure_span()


def test_verification_under_a_span(sets):
    """The CPU side of the command line's -c: the scorer with free borders equals the dynamic program on small, the CIGAR is priced
    without its free runs."""
    lib = wfagpu.load()
    span_t = C.c_int * 4
    lib.verification_cpu_score_span.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    lib.verification_cpu_score_span.restype = C.c_int
    lib.check_affine_distance_span.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p,
                                               C.POINTER(C.c_int)]
    lib.check_affine_distance_span.restype = C.c_bool
    lib.check_cigar_edit.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_char_p]
    lib.check_cigar_edit.restype = C.c_bool
    lib.verification_cpu_score.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int]
    lib.verification_cpu_score.restype = C.c_int
    g = sets["small"]
    for i, ((p, t), span, pen) in enumerate(zip(g["pairs"], g["spans"], g["pens"])):
        sp = span_t(*span)
        want = ef.dp_endsfree_score(p, t, pen, span)
        assert lib.verification_cpu_score_span(p, t, len(p), len(t), *pen, sp) == want, (i, span, pen)
        cg = g["cigars"][i].encode()
        assert lib.check_cigar_edit(t, p, len(t), len(p), cg)
        assert lib.check_affine_distance_span(t, p, len(t), len(p), int(want), *pen, cg, sp), (i, span, pen)
        assert not lib.check_affine_distance_span(t, p, len(t), len(p), int(want) + 1, *pen, cg, sp)
        if span == (0, 0, 0, 0):
            assert lib.verification_cpu_score(p, t, len(p), len(t), *pen) == want
            assert lib.verification_cpu_score_span(p, t, len(p), len(t), *pen, None) == want
