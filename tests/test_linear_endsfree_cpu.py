"""Edit, indel and gap-linear distances under an ends-free span, without a GPU: the golden files against a one-matrix dynamic program
with free borders, a plain numpy model of the search and (where the reference is compiled in place) WFA2 run live; the host-side
pieces -- the two new symbols, wfagpu_amd_configure_linear_span, the -c checkers, --metric-ends-free's usage errors, and the new host
code under the address and undefined-behaviour sanitizers as a stand-alone program."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import endsfree_ref as er
import linear_endsfree_ref as ler
import linear_ref as lr
import oracle_lib
import wfagpu

PKG = os.path.dirname(wfagpu.LIB_PATH)
ROOT = os.path.dirname(PKG)
CLI = os.path.join(PKG, "bin", "wfa.affine.gpu")
DP_SETS = ler.SETS + (ler.SWEEP_SET,)
ALL_SETS = DP_SETS + (ler.LONG_SET,)
M_ID = {"indel": 0, "edit": 1, "linear": 2}


@pytest.fixture(scope="module")
def sets():
    return {name: ler.read_golden(name) for name in ALL_SETS}


def test_golden_sets_have_the_shapes_they_are_for(sets):
    assert [len(sets[n]["pairs"]) for n in ALL_SETS] == [400, 400, 48, 32, 310, 2]
    small = sets["small"]
    kinds = {(er.SMALL_SPANS.index(tuple(s)), tuple(m)) for s, m in zip(small["spans"], small["metrics"])}
    assert len(kinds) == 54, "every span kind under every metric"
    assert sum(1 for p, t in small["pairs"] if set(p + t) - set(b"ACGT")) == 13
    t50 = sets["small_edit_t50"]
    assert set(map(tuple, t50["spans"])) == {ler.ONE_SPAN} and set(t50["metrics"]) == {lr.EDIT}
    assert sorted({s[0] + s[2] + 1 for s in sets["wide"]["spans"]}) == [63, 64, 65, 129, 257, 1025]
    assert set(sets["wide"]["metrics"]) == set(lr.LANES_METRICS) and set(sets["ties"]["metrics"]) == set(lr.TIES_METRICS)
    sweep = sets[ler.SWEEP_SET]
    assert set(sweep["metrics"]) == set(lr.SWEEP_METRICS) and set(map(tuple, sweep["spans"])) == set(er.SWEEP_SPANS)
    for m in lr.SWEEP_METRICS:      # every metric of the sweep meets every span
        assert {tuple(s) for s, mm in zip(sweep["spans"], sweep["metrics"]) if mm == m} == set(er.SWEEP_SPANS)
    assert all(len(p) > 32766 and len(t) > 32766 for p, t in sets[ler.LONG_SET]["pairs"])
    assert sum(os.path.getsize(ler.golden_path(name)) for name in ALL_SETS) < (1 << 18)


@pytest.mark.parametrize("name", DP_SETS)
def test_golden_scores_equal_the_dynamic_program_with_free_borders(sets, name):
    g = sets[name]
    for i, ((p, t), m, span) in enumerate(zip(g["pairs"], g["metrics"], g["spans"])):
        assert ler.dp_linear_endsfree_score(p, t, *lr.pens_of(m), span) == g["scores"][i], (name, i, m, span)


@pytest.mark.parametrize("name", ALL_SETS)
def test_golden_cigars_are_valid_and_cost_their_score_without_the_free_runs(sets, name):
    g = sets[name]
    for i, ((p, t), m, span) in enumerate(zip(g["pairs"], g["metrics"], g["spans"])):
        ok, cost = ler.check_cigar_linear_span(p, t, g["cigars"][i], m, span)
        assert ok and cost == g["scores"][i], (name, i, m, span)


def test_the_goldens_differ_from_the_end_to_end_answers(sets):
    """A path that ignores the span fails: the scores of most pairs are not the end-to-end ones under the same metric (half of `small`
    are reads inside a padded window, `wide` and `ties` carry free text on every pair)."""
    for name in ler.SETS:
        g = sets[name]
        differ = sum(lr.dp_linear_score(p, t, *lr.pens_of(m)) != s for (p, t), m, s in zip(g["pairs"], g["metrics"], g["scores"]))
        print(name, differ, "of", len(g["pairs"]), "scores differ from the end-to-end ones")
        assert 2 * differ > len(g["pairs"]), (name, differ)


def _model_indices(name, g):
    if name == "ties":
        return range(len(g["pairs"]))
    if name == "small":
        return range(0, len(g["pairs"]), 5)
    return [i for i, s in enumerate(g["spans"]) if s[0] + s[2] + 1 == 1025]      # wide


@pytest.mark.parametrize("name", ["ties", "small", "wide"])
def test_the_model_gives_wfa2s_bytes(sets, name):
    g = sets[name]
    idx = list(_model_indices(name, g))
    assert len(idx) == {"ties": 32, "small": 80, "wide": 8}[name]
    for i in idx:
        (p, t), m, span = g["pairs"][i], g["metrics"][i], g["spans"][i]
        s, c, ends = ler.wfa_linear_endsfree_model(p, t, m, span)
        assert s == g["scores"][i] and c == g["cigars"][i], (name, i, m, span)
        ok, cost = ler.check_cigar_linear_span(p, t, c, m, span, ends=ends)
        assert ok and cost == s, (name, i, ends)


@pytest.mark.skipif(not oracle_lib.have_ref(), reason="the reference's WFA2 is not compiled in place here")
@pytest.mark.parametrize("name", ALL_SETS)
def test_wfa2_run_live_equals_the_golden_files(sets, name):
    g = sets[name]
    scores, cigars = ler.wfa2_linear_endsfree(g["pairs"], g["metrics"], g["spans"])
    assert np.array_equal(scores, g["scores"]) and cigars == g["cigars"], name


@pytest.mark.skipif(not oracle_lib.have_ref(), reason="the reference's WFA2 is not compiled in place here")
def test_wfa2_edit_against_its_gap_affine_self_at_a_zero_opening_under_the_span(sets):
    g = sets["small_edit_t50"]
    s_em, c_em = er.wfa2_endsfree(g["pairs"], g["spans"], [ler.EMULATION_PEN] * len(g["pairs"]))
    assert np.array_equal(s_em, g["scores"])
    assert (list(c_em) == g["cigars"]) == ler.SMALL_EDIT_T50_CIGARS_AGREE


def test_new_symbols_and_header_text():
    lib = wfagpu.load()
    for sym in ("wfagpu_amd_align_device_linear_span", "wfagpu_amd_configure_linear_span"):
        assert sym in wfagpu.ABI_SYMBOLS and hasattr(lib, sym)
    header = open(os.path.join(ROOT, "include", "wfa_gpu_device.h")).read()
    assert "int wfagpu_amd_align_device_linear_span(wfagpu_amd_ctx_t* ctx, const wfagpu_amd_batch_t* batch, const wfagpu_amd_linear_t* linear, int max_error," in header
    assert "int wfagpu_amd_configure_linear_span(const wfagpu_amd_linear_t* linear, const wfagpu_amd_span_t* span);" in header
    assert "bit 6: the one-component wavefront kernels under an ends-free span" in header
    assert "WFA_UNIT_ALIGN_LINEF = 64u" in open(os.path.join(PKG, "csrc", "wfa_device.h")).read()


def test_configure_linear_span_semantics():
    lib = wfagpu.load()
    L, S = wfagpu.Linear, wfagpu.Span
    span, pen2, heur = S(0, 0, 5, 5), wfagpu.Penalties2p(4, 6, 2, 24, 1), wfagpu.WfAdaptive(10, 50, 1)
    cfg = lib.wfagpu_amd_configure_linear_span
    try:
        assert cfg(C.byref(L(1, 0, 0)), C.byref(span)) == 0
        # while it holds, the three existing calls still return -1
        assert lib.wfagpu_amd_configure_span(C.byref(span)) == -1
        assert lib.wfagpu_amd_configure_affine2p(C.byref(pen2)) == -1
        assert lib.wfagpu_amd_configure_wfadaptive(C.byref(heur)) == -1
        # negative members and bad metrics are rejected
        for bad in ((-1, 0, 0, 0), (0, -1, 0, 0), (0, 0, -1, 0), (0, 0, 0, -1)):
            assert cfg(C.byref(L(1, 0, 0)), C.byref(S(*bad))) == -1
        for bad in ((3, 1, 1), (2, 0, 1), (2, 4, 0)):
            assert cfg(C.byref(L(*bad)), C.byref(span)) == -1
        assert cfg(C.byref(L(2, 4, 2)), None) == 0                    # a NULL span: end to end
        assert cfg(C.byref(L(0, 0, 0)), C.byref(S(0, 0, 0, 0))) == 0
        # configure_linear(NULL) clears the span with the metric: the gap-affine span is free to be set again
        assert lib.wfagpu_amd_configure_linear(None) == 0
        assert lib.wfagpu_amd_configure_span(C.byref(span)) == 0 and lib.wfagpu_amd_configure_span(None) == 0
        assert cfg(C.byref(L(1, 0, 0)), C.byref(span)) == 0
        assert cfg(None, C.byref(span)) == 0                           # linear == NULL clears both, whatever the span
        assert lib.wfagpu_amd_configure_affine2p(C.byref(pen2)) == 0 and lib.wfagpu_amd_configure_affine2p(None) == 0
        # the other way round: -1 while one of the three holds, and their state stays
        for conf, arg in ((lib.wfagpu_amd_configure_span, span), (lib.wfagpu_amd_configure_affine2p, pen2), (lib.wfagpu_amd_configure_wfadaptive, heur)):
            assert conf(C.byref(arg)) == 0
            assert cfg(C.byref(L(1, 0, 0)), C.byref(span)) == -1
            assert lib.wfagpu_amd_configure_linear(C.byref(L(1, 0, 0))) == -1      # (so the metric was not set by the refused call)
            assert conf(C.byref(arg)) == 0      # (still the one configured: setting it again is no conflict)
            assert conf(None) == 0
        wfagpu.configure_linear(("edit",), span=(0, 0, 50, 50))
        wfagpu.configure_linear(("linear", 4, 2), span={"text_begin_free": 3})
        with pytest.raises(ValueError):
            wfagpu.configure_linear(("edit",), span=(0, 0, -1, 0))
        with pytest.raises(ValueError):
            wfagpu.configure_linear(("linear", 0, 2), span=(0, 0, 1, 0))
    finally:
        wfagpu.configure_linear()
        wfagpu.configure_wfadaptive()
        wfagpu.configure_affine2p()
        wfagpu.configure_span()


def test_the_checkers_of_the_check_flag(sets):
    lib = wfagpu.load()
    lib.check_linear_distance_span.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_int)]
    lib.check_linear_distance_span.restype = C.c_bool
    lib.verification_cpu_score_linear_span.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    lib.verification_cpu_score_linear_span.restype = C.c_int
    sp = lambda s: (C.c_int * 4)(*[min(int(v), er.INT_MAX) for v in s])
    p, t = b"ACGTACGTAC", b"TTTACCTACGGTACAA"      # 3 bases, the pattern with one mismatch and one inserted G, 2 bases
    cg = b"3I2M1X4M1I3M2I"
    check = lambda dist, metric, x, g, span, c=cg: lib.check_linear_distance_span(t, p, len(t), len(p), dist, metric, x, g, c, sp(span))
    assert check(2, 1, 0, 0, (0, 0, 5, 5)) and not check(3, 1, 0, 0, (0, 0, 5, 5))
    assert check(4, 1, 0, 0, (0, 0, 2, 1)) and not check(2, 1, 0, 0, (0, 0, 2, 1))      # free runs longer than allowed are paid for
    assert check(7, 1, 0, 0, (0, 0, 0, 0)) and check(6, 2, 4, 2, (0, 0, 5, 5))
    assert not check(2, 0, 0, 0, (0, 0, 5, 5)) and not check(3, 0, 0, 0, (0, 0, 5, 5))     # indel: an X is a failure whatever the distance
    assert check(3, 0, 0, 0, (0, 0, 5, 5), b"3I2M1I1D4M1I3M2I")
    assert not check(2, 1, 0, 0, (0, 0, 5, 5), b"3I2M1Y4M1I3M2I") and not check(2, 3, 1, 1, (0, 0, 5, 5))
    score = lambda metric, x, g, span: lib.verification_cpu_score_linear_span(p, t, len(p), len(t), metric, x, g, sp(span))
    assert (score(1, 0, 0, (0, 0, 5, 5)), score(0, 0, 0, (0, 0, 5, 5)), score(2, 4, 2, (0, 0, 5, 5)), score(1, 0, 0, (0, 0, 2, 1))) == (2, 3, 6, 4)
    assert score(1, 0, 0, (0, 0, 0, 0)) == ler.dp_linear_endsfree_score(p, t, 1, 1, (0, 0, 0, 0)) == lr.dp_linear_score(p, t, 1, 1)
    assert score(3, 1, 1, (0, 0, 5, 5)) == -1
    for name in ("ties", "small"):
        g = sets[name]
        for i in range(0, len(g["pairs"]), 5 if name == "small" else 1):
            (pp, tt), m, span = g["pairs"][i], g["metrics"][i], g["spans"][i]
            x, gg = (m[1], m[2]) if m[0] == "linear" else (0, 0)
            assert lib.verification_cpu_score_linear_span(pp, tt, len(pp), len(tt), M_ID[m[0]], x, gg, sp(span)) == g["scores"][i], (name, i, m, span)
            assert lib.check_linear_distance_span(tt, pp, len(tt), len(pp), int(g["scores"][i]), M_ID[m[0]], x, gg, g["cigars"][i].encode(), sp(span)), (name, i, m, span)


@pytest.mark.parametrize("args", [["--metric-ends-free", "0,0,5,5"], ["--edit", "--metric-ends-free", "0,0,5,5", "-B", "10"],
                                  ["--edit", "--metric-ends-free", "0,0,5,5", "--ends-free", "0,0,5,5"], ["--indel", "--metric-ends-free", "0,0,5"],
                                  ["--gap-linear", "4,2", "--metric-ends-free", "0,0,5,5x"], ["--edit", "--metric-ends-free", "0,0,-5,5"],
                                  ["--edit", "--indel", "--metric-ends-free", "0,0,5,5"], ["--edit", "--metric-ends-free", "0,0,5,5", "--affine2p", "4,6,2,24,1"],
                                  ["--edit", "--metric-ends-free", "0,0,5,5", "--wfa-adaptive", "10,50,1"]])
def test_cli_usage_errors_come_before_any_device_work(args, golden_dir):
    seq = os.path.join(golden_dir, "seq1k.seq")
    r = subprocess.run([CLI, "-i", seq] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    errors = [line for line in r.stderr.splitlines() if "ERROR" in line]
    assert errors and "--metric-ends-free" in errors[0], r.stderr[-2000:]
    assert "--metric-ends-free <pb,pe,tb,te>" in r.stdout + r.stderr      # (the usage text, next to the other options')
    assert "HIP device" not in r.stderr and "Reading sequences" not in r.stdout + r.stderr


def test_new_host_code_under_address_and_ub_sanitizers(tmp_path):
    """utils/verification.c's span checkers and the option's parser, in a stand-alone program: nothing is loaded into Python."""
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    exe = str(tmp_path / "linef_host_asan")
    b = subprocess.run(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-I", os.path.join(ROOT, "include"), "-I", PKG, os.path.join(ROOT, "tests", "linef_host_asan.c"),
                        os.path.join(PKG, "utils", "verification.c"), "-lm", "-o", exe], capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "linef_host_asan ok" in run.stdout, (run.stdout + run.stderr)[-4000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]
