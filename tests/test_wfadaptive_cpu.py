"""The wf-adaptive heuristic without a GPU: the golden files against the exact optimum and (where the reference is compiled in place)
against WFA2 run live; the host-side pieces -- the new symbols, wfagpu_amd_configure_wfadaptive, the relaxed -c verdict, the command
line's usage errors."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import oracle_lib
import wfadaptive_ref as wa
import wfagpu

PKG = os.path.dirname(wfagpu.LIB_PATH)
CLI = os.path.join(PKG, "bin", "wfa.affine.gpu")


@pytest.fixture(scope="module")
def sets():
    return {name: wa.read_golden(name) for name in wa.ALL_SETS + (wa.SWEEP_SET,)}


def test_golden_sets_have_the_shapes_they_are_for(sets):
    small, indel, d1k, long_, b16 = (sets[n] for n in wa.SETS)
    assert [len(sets[n]["pairs"]) for n in wa.ALL_SETS] == [400, 64, 48, 8, 2, 400]
    assert any(len(p) == 0 for p, _ in small["pairs"]) and any(len(t) == 0 for _, t in small["pairs"])
    assert any(p == t and len(p) > 0 for p, t in small["pairs"])
    assert max(max(len(p), len(t)) for p, t in small["pairs"]) <= 300
    assert 8 <= sum(1 for p, t in small["pairs"] if set(p + t) - set(b"ACGT")) <= 16
    assert set(small["heurs"]) == set(wa.SMALL_HEUR) and set(small["pens"]) == set(wa.PENS)
    assert set(indel["heurs"]) == {(4, 5, 3)} and all(850 <= len(s) <= 1200 for pair in indel["pairs"] for s in pair)
    assert set(d1k["heurs"]) == {(10, 50, 1), (10, 50, 10)}
    assert sum(1 for p, t in d1k["pairs"] if (len(p), len(t)) == (1000, 1000)) == 24
    assert sum(1 for p, t in d1k["pairs"] if (len(p), len(t)) == (600, 900)) == 24
    assert set(long_["heurs"]) == {(10, 10, 1), (64, 20, 1)} and all(4000 <= len(s) <= 6000 for pair in long_["pairs"] for s in pair)
    assert all(len(p) > 32766 and len(t) > 32766 for p, t in b16["pairs"]) and set(b16["heurs"]) == {wa.DEFAULTS}
    one = sets[wa.ONE_SET]
    assert one["pairs"] == small["pairs"] and set(one["heurs"]) == {wa.ONE_HEUR} and set(one["pens"]) == {wa.ONE_PEN}
    assert sum(os.path.getsize(wa.golden_path(name)) for name in wa.ALL_SETS) < (1 << 20)


def test_the_sweep_has_the_shape_it_is_for(sets):
    """7 penalty sets of 20 short pairs each, four under each of the five heuristics, and 5 long pairs -- one per heuristic -- under M rings
    of 8 and 66 rows; every penalty set has its byte-compare pair and its empty side; a deep ring gets short pairs."""
    g = sets[wa.SWEEP_SET]
    groups = wa.groups(g)
    assert len(g["pairs"]) == 7 * 20 + 2 * 5 and len(wa.SWEEP_PENS) == 7 and len(wa.SWEEP_HEUR) == 5
    assert set(groups) == {(h, pen) for h in wa.SWEEP_HEUR for pen in wa.SWEEP_PENS}
    depth = wa.ring_depth
    assert sorted(depth(pen) for pen in wa.SWEEP_PENS)[-3:] == [41, 64, 66] and sum(1 for pen in wa.SWEEP_PENS if math.gcd(*pen) > 1) == 1
    assert sorted(depth(pen) for pen in wa.SWEEP_LONG_PENS) == [8, 66]
    for pen in wa.SWEEP_PENS:
        idx = [i for i, q in enumerate(g["pens"]) if q == pen]
        short = [g["pairs"][i] for i in idx[:20]]
        assert len(idx) == (25 if pen in wa.SWEEP_LONG_PENS else 20)
        assert all(600 <= len(p) <= 800 and 600 <= len(t) <= 800 for p, t in (g["pairs"][i] for i in idx[20:]))
        assert sum(1 for p, t in short if set(p + t) - set(b"ACGT")) == 1 and sum(1 for p, t in short if not p or not t) == 1
        assert max(max(len(p), len(t)) for p, t in short) <= (48 if depth(pen) >= 60 else 160)
    assert any(not p for p, _ in g["pairs"]) and any(not t for _, t in g["pairs"])
    assert os.path.getsize(wa.golden_path(wa.SWEEP_SET)) < (64 << 10)


@pytest.mark.parametrize("name", sorted(wa.MIN_DIFFERENT))
def test_the_heuristic_changes_answers_in_the_sets_that_are_meant_to_show_it(sets, name):
    """A heuristic test proves nothing where the heuristic changes nothing: pairs whose stored score lies above the exact optimum
    (defaults1k: or whose CIGAR differs from the exact one), counted from the stored files with the C oracle alone."""
    assert wa.count_different(sets[name], cigars_too=name == "defaults1k") >= wa.MIN_DIFFERENT[name]


@pytest.mark.parametrize("name", wa.ALL_SETS + (wa.SWEEP_SET,))
def test_golden_cigars_are_valid_cost_their_score_and_no_score_is_below_the_optimum(sets, name):
    g = sets[name]
    opt, _ = wa.exact_answers(g["pairs"], g["pens"])
    for i, ((p, t), pen) in enumerate(zip(g["pairs"], g["pens"])):
        ok, cost = oracle_lib.check_cigar(p, t, g["cigars"][i], pen)
        assert ok and cost == g["scores"][i], (name, i, pen)
        assert g["scores"][i] >= opt[i], (name, i, pen)


@pytest.mark.skipif(not oracle_lib.have_ref(), reason="the reference's WFA2 is not compiled in place here")
@pytest.mark.parametrize("name", wa.ALL_SETS + (wa.SWEEP_SET,))
def test_wfa2_run_live_equals_the_golden_files(sets, name):
    g = sets[name]
    scores, cigars = wa.wfa2_wfadaptive(g["pairs"], g["heurs"], g["pens"])
    assert np.array_equal(scores, g["scores"]) and cigars == g["cigars"], name


@pytest.mark.skipif(not oracle_lib.have_ref(), reason="the reference's WFA2 is not compiled in place here")
def test_wfa2_under_a_heuristic_that_never_cuts_equals_its_exact_self(sets):
    """(1, 1 << 20, 1): a cut-off at every score that drops nothing -- what the GPU identity tests rely on."""
    for name in ("small", "indel"):
        g = sets[name]
        scores, cigars = wa.wfa2_wfadaptive(g["pairs"], [(1, 1 << 20, 1)] * len(g["pairs"]), g["pens"])
        opt, exact = wa.exact_answers(g["pairs"], g["pens"], cigar=True)
        assert np.array_equal(scores, opt) and cigars == exact, name


def test_new_symbols_and_the_heuristic_struct():
    lib = wfagpu.load()
    for sym in ("wfagpu_amd_align_device_adaptive", "wfagpu_amd_configure_wfadaptive"):
        assert sym in wfagpu.ABI_SYMBOLS and hasattr(lib, sym)
    assert C.sizeof(wfagpu.WfAdaptive) == 3 * C.sizeof(C.c_int)
    assert [f for f, _ in wfagpu.WfAdaptive._fields_] == ["min_wavefront_length", "max_distance_threshold", "steps_between_cutoffs"]
    header = open(os.path.join(os.path.dirname(PKG), "include", "wfa_gpu_device.h")).read()
    assert "typedef struct { int min_wavefront_length, max_distance_threshold, steps_between_cutoffs; } wfagpu_amd_wfadaptive_t;" in header


def test_configure_wfadaptive_rejects_bad_members_and_the_exclusions_leave_the_state_alone():
    lib = wfagpu.load()
    H = wfagpu.WfAdaptive
    try:
        assert lib.wfagpu_amd_configure_wfadaptive(C.byref(H(10, 50, 1))) == 0
        for bad in ((0, 50, 1), (-3, 50, 1), (10, -1, 1), (10, 50, 0), (10, 50, -2)):
            assert lib.wfagpu_amd_configure_wfadaptive(C.byref(H(*bad))) == -1
        assert lib.wfagpu_amd_configure_wfadaptive(C.byref(H(1, 0, 1))) == 0      # (the smallest values WFA2 makes sense of)
        # still configured: a span and two-piece penalties are refused while it is
        assert lib.wfagpu_amd_configure_span(C.byref(wfagpu.Span(0, 0, 5, 5))) == -1
        assert lib.wfagpu_amd_configure_affine2p(C.byref(wfagpu.Penalties2p(4, 6, 2, 24, 1))) == -1
        assert lib.wfagpu_amd_configure_wfadaptive(None) == 0
        # and the other way round: refused while a span, or two-piece penalties, are configured; their state stays
        assert lib.wfagpu_amd_configure_span(C.byref(wfagpu.Span(0, 0, 5, 5))) == 0
        assert lib.wfagpu_amd_configure_wfadaptive(C.byref(H(10, 50, 1))) == -1
        assert lib.wfagpu_amd_configure_affine2p(C.byref(wfagpu.Penalties2p(4, 6, 2, 24, 1))) == -1      # (the span is still there)
        assert lib.wfagpu_amd_configure_span(None) == 0
        assert lib.wfagpu_amd_configure_affine2p(C.byref(wfagpu.Penalties2p(4, 6, 2, 24, 1))) == 0
        assert lib.wfagpu_amd_configure_wfadaptive(C.byref(H(10, 50, 1))) == -1
        assert lib.wfagpu_amd_configure_span(C.byref(wfagpu.Span(0, 0, 5, 5))) == -1                      # (the penalties are still there)
        assert lib.wfagpu_amd_configure_affine2p(None) == 0
        with pytest.raises(ValueError):
            wfagpu.configure_wfadaptive((10, 50, 0))
        wfagpu.configure_wfadaptive((10, 50, 1))
    finally:
        wfagpu.configure_wfadaptive()
        wfagpu.configure_affine2p()
        wfagpu.configure_span()


def test_the_relaxed_verdict_of_the_check_flag(sets):
    """The CPU side of the command line's -c under the heuristic: the CIGAR checkers as they are (valid, costs the score); the score
    against the CPU scorer's optimum: equal 0, above its excess (counted, no failure), below -1 (a failure)."""
    lib = wfagpu.load()
    lib.verification_heuristic_verdict.argtypes = [C.c_int, C.c_int]
    lib.verification_heuristic_verdict.restype = C.c_int
    lib.verification_cpu_score.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int]
    lib.verification_cpu_score.restype = C.c_int
    lib.check_affine_distance.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p]
    lib.check_affine_distance.restype = C.c_bool
    lib.check_cigar_edit.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_char_p]
    lib.check_cigar_edit.restype = C.c_bool
    assert lib.verification_heuristic_verdict(10, 10) == 0
    assert lib.verification_heuristic_verdict(17, 10) == 7
    assert lib.verification_heuristic_verdict(9, 10) == -1
    g = sets["indel"]
    above = 0
    for i, ((p, t), pen) in enumerate(zip(g["pairs"], g["pens"])):
        cg = g["cigars"][i].encode()
        score = int(g["scores"][i])
        assert lib.check_cigar_edit(t, p, len(t), len(p), cg)
        assert lib.check_affine_distance(t, p, len(t), len(p), score, *pen, cg), (i, pen)
        verdict = lib.verification_heuristic_verdict(score, lib.verification_cpu_score(p, t, len(p), len(t), *pen))
        assert verdict >= 0, (i, pen)
        above += verdict > 0
    assert above >= wa.MIN_DIFFERENT["indel"]


@pytest.mark.parametrize("args", [["--wfa-adaptive", "10,50"], ["--wfa-adaptive", "0,50,1"], ["--wfa-adaptive", "10,-1,1"],
                                  ["--wfa-adaptive", "10,50,0"], ["--wfa-adaptive", "10,50,1x"], ["--wfa-adaptive", "10,50,1", "-B", "10"],
                                  ["--wfa-adaptive", "10,50,1", "--ends-free", "0,0,5,5"],
                                  ["--wfa-adaptive", "10,50,1", "--affine2p", "4,6,2,24,1"]])
def test_cli_usage_errors_come_before_any_device_work(args, golden_dir):
    seq = os.path.join(golden_dir, "seq1k.seq")
    r = subprocess.run([CLI, "-i", seq] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "--wfa-adaptive" in r.stderr and "ERROR" in r.stderr
    assert "HIP device" not in r.stderr and "Reading sequences" not in r.stdout + r.stderr
