"""Edit, indel and gap-linear distances without a GPU: the golden files against a one-matrix dynamic program, a plain numpy model of the
M-only wavefront search and (where the reference is compiled in place) WFA2 run live; the host-side pieces -- the new symbols,
wfagpu_amd_configure_linear, the -c checkers, the command line's usage errors."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import linear_ref as lr
import oracle_lib
import wfagpu

PKG = os.path.dirname(wfagpu.LIB_PATH)
CLI = os.path.join(PKG, "bin", "wfa.affine.gpu")
ALL_SETS = lr.SETS + (lr.LONG_SET,)


@pytest.fixture(scope="module")
def sets():
    return {name: lr.read_golden(name) for name in ALL_SETS + (lr.SWEEP_SET,)}


def test_golden_sets_have_the_shapes_they_are_for(sets):
    assert [len(sets[n]["pairs"]) for n in ALL_SETS] == [400, 400, 32, 24, 6, 2]
    small = sets["small"]
    assert any(len(p) == 0 for p, _ in small["pairs"]) and any(len(t) == 0 for _, t in small["pairs"])
    assert any(p == t and len(p) > 0 for p, t in small["pairs"])
    assert sum(1 for p, t in small["pairs"] if set(p + t) - set(b"ACGT")) == 13
    assert set(small["metrics"]) == set(lr.METRICS) and set(sets["small_edit"]["metrics"]) == {lr.EDIT}
    assert sets["small_edit"]["pairs"] == small["pairs"]
    assert set(sets["ties"]["metrics"]) == set(lr.TIES_METRICS) and set(sets["lanes"]["metrics"]) == set(lr.LANES_METRICS)
    assert all(1050 <= len(s) <= 1350 for pair in sets["lanes"]["pairs"] for s in pair)
    wide = sets["wide"]
    assert [(len(p), len(t)) for p, t in wide["pairs"]] == [(600, 3000), (3000, 600), (2500, 2600), (1500, 1500), (600, 3000), (3000, 600)]
    assert wide["metrics"] == [lr.EDIT] * 4 + [lr.INDEL] * 2
    # (edit rows of these pairs pass 1000 diagonals, where WFA2's exact pruning is active: a row of score s spans up to 2 s + 1, bounded
    # by the plen + tlen + 1 diagonals there are)
    assert all(min(2 * int(s) + 1, len(p) + len(t) + 1) > 1000 for s, (p, t) in zip(wide["scores"], wide["pairs"]))
    assert all(len(p) > 32766 and len(t) > 32766 for p, t in sets[lr.LONG_SET]["pairs"])
    assert sum(os.path.getsize(lr.golden_path(name)) for name in ALL_SETS) < (1 << 20)


def test_no_x_in_a_golden_indel_cigar_and_indel_is_not_gap_linear_2_1(sets):
    g = sets["small"]
    idx = [i for i, m in enumerate(g["metrics"]) if m == lr.INDEL]
    assert idx and all("X" not in g["cigars"][i] for i in idx)
    differ = 0
    for i in idx:
        p, t = g["pairs"][i]
        s21, c21 = lr.wfa_linear_model(p, t, ("linear", 2, 1))
        assert s21 == g["scores"][i]
        differ += c21 != g["cigars"][i]
    assert 4 * differ >= len(idx)


def test_the_sweep_has_the_shape_it_is_for(sets):
    """15 metrics of 20 short pairs each and 5 long pairs on either side of the one-wave tier's ring depth; every metric has its
    byte-compare pair and its empty side; the planted gaps start at one base, alternate sides and reach 60 bases where the pairs are
    long enough; a deep ring gets short pairs (endsfree_ref.sweep_top)."""
    g = sets[lr.SWEEP_SET]
    groups = lr.groups(g)
    assert len(g["pairs"]) == 15 * 20 + 2 * 5 and set(groups) == set(lr.SWEEP_METRICS) and len(lr.SWEEP_METRICS) == 15
    assert sorted(lr.ring_depth(m) for m in lr.SWEEP_LONG_METRICS) == [64, 65]
    assert sorted(lr.ring_depth(m) for m in lr.SWEEP_METRICS)[-7:] == [41, 64, 64, 65, 65, 66, 66]
    assert {math.gcd(m[1], m[2]) for m in lr.SWEEP_METRICS} == {1, 3, 9}
    for m, idx in groups.items():
        short = [g["pairs"][i] for i in idx if max(map(len, g["pairs"][i])) <= 160]
        assert len(short) == 20 and len(idx) == (25 if m in lr.SWEEP_LONG_METRICS else 20)
        assert all(600 <= len(p) <= 800 and 600 <= len(t) <= 800 for p, t in (g["pairs"][i] for i in idx[20:]))
        assert sum(1 for p, t in short if set(p + t) - set(b"ACGT")) == 1 and sum(1 for p, t in short if not p or not t) == 1
        assert max(max(len(p), len(t)) for p, t in short) <= (48 if lr.ring_depth(m) >= 60 else 160)
        gaps = [abs(len(p) - len(t)) for p, t in short[12:16]]
        assert gaps[0] == 1 and gaps[1] == max(gaps) and (gaps[1] == 60 or lr.ring_depth(m) >= 60)
        assert [len(p) < len(t) for p, t in short[12:16]] == [True, False, True, False]
    assert any(not p for p, _ in g["pairs"]) and any(not t for _, t in g["pairs"])
    assert os.path.getsize(lr.golden_path(lr.SWEEP_SET)) < (64 << 10)


@pytest.mark.parametrize("name", ["small", "ties", "lanes", lr.SWEEP_SET])
def test_golden_scores_equal_the_dynamic_program(sets, name):
    g = sets[name]
    for i, ((p, t), m) in enumerate(zip(g["pairs"], g["metrics"])):
        assert lr.dp_linear_score(p, t, *lr.pens_of(m)) == g["scores"][i], (name, i, m)


@pytest.mark.parametrize("name", ALL_SETS + (lr.SWEEP_SET,))
def test_golden_cigars_are_valid_and_cost_their_score(sets, name):
    g = sets[name]
    for i, ((p, t), m) in enumerate(zip(g["pairs"], g["metrics"])):
        ok, cost = lr.check_cigar_linear(p, t, g["cigars"][i], m)
        assert ok and cost == g["scores"][i], (name, i, m)


@pytest.mark.parametrize("name", lr.SETS + (lr.SWEEP_SET,))
def test_the_model_without_pruning_gives_wfa2s_bytes(sets, name):
    """No exact pruning of wide edit rows, mismatch > deletion > insertion on equal offsets: what the kernels restate."""
    g = sets[name]
    for i, ((p, t), m) in enumerate(zip(g["pairs"], g["metrics"])):
        s, c = lr.wfa_linear_model(p, t, m)
        assert s == g["scores"][i] and c == g["cigars"][i], (name, i, m)


@pytest.mark.skipif(not oracle_lib.have_ref(), reason="the reference's WFA2 is not compiled in place here")
@pytest.mark.parametrize("name", ALL_SETS + (lr.SWEEP_SET,))
def test_wfa2_run_live_equals_the_golden_files(sets, name):
    g = sets[name]
    scores, cigars = lr.wfa2_linear(g["pairs"], g["metrics"])
    assert np.array_equal(scores, g["scores"]) and cigars == g["cigars"], name


@pytest.mark.skipif(not oracle_lib.have_ref(), reason="the reference's WFA2 is not compiled in place here")
def test_wfa2_agrees_with_its_gap_affine_self_at_a_zero_opening(golden_dir):
    """WFA2 gap-linear (x, g) against WFA2 gap-affine (x, 0, g), edit against (1, 0, 1), on seq1k.seq: the scores agree; whether the
    CIGAR bytes do is recorded in linear_ref.SEQ1K_CIGARS_AGREE (they do), which the GPU cross-check follows."""
    pairs = wfagpu.read_seq_file(os.path.join(golden_dir, "seq1k.seq"))
    buf, meta = wfagpu.layout_pairs(pairs)
    agree = True
    for metric, pen in lr.SEQ1K_CROSS:
        s_aff, c_aff = oracle_lib.ref_batch(buf, meta, pen, cigar=True)
        s_lin, c_lin = lr.wfa2_linear(pairs, [metric] * len(pairs))
        assert np.array_equal(s_aff, s_lin), metric
        agree &= list(c_aff) == list(c_lin)
    assert agree == lr.SEQ1K_CIGARS_AGREE


def test_new_symbols_and_the_metric_struct():
    lib = wfagpu.load()
    for sym in ("wfagpu_amd_align_device_linear", "wfagpu_amd_configure_linear"):
        assert sym in wfagpu.ABI_SYMBOLS and hasattr(lib, sym)
    assert C.sizeof(wfagpu.Linear) == 3 * C.sizeof(C.c_int)
    assert [f for f, _ in wfagpu.Linear._fields_] == ["metric", "mismatch", "indel"]
    assert (wfagpu.METRIC_INDEL, wfagpu.METRIC_EDIT, wfagpu.METRIC_GAP_LINEAR) == (0, 1, 2) == tuple(lr.WFA2_METRIC[k] for k in ("indel", "edit", "linear"))
    header = open(os.path.join(os.path.dirname(PKG), "include", "wfa_gpu_device.h")).read()
    assert "typedef struct { int metric, mismatch, indel; } wfagpu_amd_linear_t;" in header
    assert "typedef enum { WFAGPU_AMD_METRIC_INDEL = 0, WFAGPU_AMD_METRIC_EDIT = 1, WFAGPU_AMD_METRIC_GAP_LINEAR = 2 } wfagpu_amd_metric_t;" in header


def test_configure_linear_rejects_bad_members_and_the_exclusions_leave_the_state_alone():
    lib = wfagpu.load()
    L = wfagpu.Linear
    span, pen2, heur = wfagpu.Span(0, 0, 5, 5), wfagpu.Penalties2p(4, 6, 2, 24, 1), wfagpu.WfAdaptive(10, 50, 1)
    try:
        assert lib.wfagpu_amd_configure_linear(C.byref(L(1, 0, 0))) == 0          # edit: mismatch and indel are not read
        assert lib.wfagpu_amd_configure_linear(C.byref(L(0, -7, -7))) == 0        # indel: the same
        for bad in ((3, 1, 1), (-1, 1, 1), (2, 0, 1), (2, 4, 0), (2, -4, 2), (2, 4, -2)):
            assert lib.wfagpu_amd_configure_linear(C.byref(L(*bad))) == -1
        assert lib.wfagpu_amd_configure_linear(C.byref(L(2, 4, 2))) == 0
        # still configured: a span, two-piece penalties and the heuristic are refused while it is
        assert lib.wfagpu_amd_configure_span(C.byref(span)) == -1
        assert lib.wfagpu_amd_configure_affine2p(C.byref(pen2)) == -1
        assert lib.wfagpu_amd_configure_wfadaptive(C.byref(heur)) == -1
        assert lib.wfagpu_amd_configure_linear(None) == 0
        # and the other way round: refused while one of them is configured; their state stays
        for conf, arg in ((lib.wfagpu_amd_configure_span, span), (lib.wfagpu_amd_configure_affine2p, pen2), (lib.wfagpu_amd_configure_wfadaptive, heur)):
            assert conf(C.byref(arg)) == 0
            assert lib.wfagpu_amd_configure_linear(C.byref(L(1, 0, 0))) == -1
            assert conf(C.byref(arg)) == 0      # (still the one configured: setting it again is no conflict)
            assert conf(None) == 0
        assert lib.wfagpu_amd_configure_linear(C.byref(L(1, 0, 0))) == 0
        assert lib.wfagpu_amd_configure_linear(None) == 0
        for bad in (("edit", 1), ("linear", 4), ("linear", 0, 2), ("levenshtein",)):
            with pytest.raises(ValueError):
                wfagpu.configure_linear(bad)
        wfagpu.configure_linear(("linear", 4, 2))
        wfagpu.configure_linear(("indel",))
    finally:
        wfagpu.configure_linear()
        wfagpu.configure_wfadaptive()
        wfagpu.configure_affine2p()
        wfagpu.configure_span()


def test_the_checkers_of_the_check_flag(sets):
    """check_linear_distance prices a CIGAR under the metric (an X under indel is a failure); verification_cpu_score_linear is a
    one-table scalar program."""
    lib = wfagpu.load()
    lib.check_linear_distance.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p]
    lib.check_linear_distance.restype = C.c_bool
    lib.verification_cpu_score_linear.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int]
    lib.verification_cpu_score_linear.restype = C.c_int
    p, t = b"ACGTACGTAC", b"ACCTACGGTAC"       # one mismatch, one inserted G
    cg = b"2M1X4M1I3M"
    check = lambda dist, metric, x, g, c=cg: lib.check_linear_distance(t, p, len(t), len(p), dist, metric, x, g, c)
    assert check(2, 1, 0, 0) and not check(3, 1, 0, 0)                 # edit: 1 + 1
    assert check(6, 2, 4, 2) and check(8, 2, 5, 3) and not check(6, 2, 5, 3)
    assert not check(2, 0, 0, 0) and not check(3, 0, 0, 0)             # indel: an X is a failure whatever the distance
    assert check(3, 0, 0, 0, b"2M1I1D4M1I3M")                           # the same alignment without the X
    assert not check(2, 1, 0, 0, b"2M1Y4M1I3M") and not check(2, 3, 1, 1) and not check(6, 2, 0, 2) and not check(6, 2, 4, 0)
    score = lambda metric, x, g: lib.verification_cpu_score_linear(p, t, len(p), len(t), metric, x, g)
    assert (score(1, 0, 0), score(0, 0, 0), score(2, 4, 2), score(2, 5, 1), score(2, 1, 3)) == (2, 3, 6, 3, 4)
    assert score(3, 1, 1) == -1 and score(2, 0, 1) == -1
    assert lib.verification_cpu_score_linear(b"", b"ACGT", 0, 4, 2, 4, 2) == 8 and lib.verification_cpu_score_linear(b"ACGT", b"ACGT", 4, 4, 0, 0, 0) == 0
    m_id = {"indel": 0, "edit": 1, "linear": 2}
    for name in ("ties", "small"):
        g = sets[name]
        for i in range(0, len(g["pairs"]), 5 if name == "small" else 1):
            (pp, tt), m = g["pairs"][i], g["metrics"][i]
            x, gg = (m[1], m[2]) if m[0] == "linear" else (0, 0)
            assert lib.verification_cpu_score_linear(pp, tt, len(pp), len(tt), m_id[m[0]], x, gg) == g["scores"][i], (name, i, m)
            assert lib.check_linear_distance(tt, pp, len(tt), len(pp), int(g["scores"][i]), m_id[m[0]], x, gg, g["cigars"][i].encode()), (name, i, m)


@pytest.mark.parametrize("args", [["--edit", "--indel"], ["--edit", "--gap-linear", "4,2"], ["--gap-linear", "4"], ["--gap-linear", "0,2"],
                                  ["--gap-linear", "4,-2"], ["--gap-linear", "4,2x"], ["--edit", "-g", "2,3,1"], ["--indel", "-B", "10"],
                                  ["--edit", "--ends-free", "0,0,5,5"], ["--gap-linear", "4,2", "--affine2p", "4,6,2,24,1"],
                                  ["--indel", "--wfa-adaptive", "10,50,1"]])
def test_cli_usage_errors_come_before_any_device_work(args, golden_dir):
    seq = os.path.join(golden_dir, "seq1k.seq")
    r = subprocess.run([CLI, "-i", seq] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "--gap-linear" in r.stderr and "ERROR" in r.stderr
    assert "HIP device" not in r.stderr and "Reading sequences" not in r.stdout + r.stderr
