"""Two-piece penalties under an ends-free span without a GPU: the goldens against the dynamic program and the CIGAR checker, the two
checkers of the command line's -c, wfagpu_amd_configure_affine2p_span, and the CLI's usage errors."""
import ctypes as C
import os
import subprocess

import pytest

import affine2p_endsfree_ref as r2
import wfagpu

CLI = os.path.join(os.path.dirname(wfagpu.LIB_PATH), "bin", "wfa.affine.gpu")


@pytest.mark.parametrize("name", ["small", "gaps", "ties"])
def test_goldens_against_the_dynamic_program_and_the_checkers(name):
    """WFA2's score equals the five-matrix program with free borders, check_cigar2p_span prices WFA2's CIGAR at that score, and
    verification.c's two new checkers agree with both."""
    lib = wfagpu.load()
    lib.verification_cpu_score_2p_span.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t] + [C.c_int] * 5 + [C.POINTER(C.c_int)]
    lib.verification_cpu_score_2p_span.restype = C.c_int
    lib.check_affine2p_distance_span.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t] + [C.c_int] * 6 + [C.c_char_p, C.POINTER(C.c_int)]
    lib.check_affine2p_distance_span.restype = C.c_bool
    g = r2.read_golden(name)
    merged = 0
    for i, ((p, t), pen, span) in enumerate(zip(g["pairs"], g["pens"], g["spans"])):
        want, cg = int(g["scores"][i]), g["cigars"][i]
        assert r2.dp_affine2p_endsfree_score(p, t, pen, span) == want, (name, i, pen, span)
        assert r2.check_cigar2p_span(p, t, cg, pen, span) == (True, want), (name, i, pen, span, cg)
        sp = (C.c_int * 4)(*span)
        assert lib.verification_cpu_score_2p_span(p, t, len(p), len(t), *pen, sp) == want, (name, i)
        assert lib.check_affine2p_distance_span(t, p, len(t), len(p), want, *pen, cg.encode(), sp), (name, i, cg)
        assert not lib.check_affine2p_distance_span(t, p, len(t), len(p), want + 1, *pen, cg.encode(), sp)
        items = r2.parse_cigar(cg)
        merged += name == "gaps" and bool(items) and max(items[0][0] if items[0][1] in "ID" else 0, items[-1][0] if items[-1][1] in "ID" else 0) > r2.GAPS_FREE
    assert name != "gaps" or merged >= 12      # (a free run and a paid run of the same kind merged in the CIGAR)


def test_configure_affine2p_span_accepts_and_rejects_and_leaves_the_state_alone():
    lib = wfagpu.load()
    pen, span = wfagpu.Penalties2p(4, 6, 2, 24, 1), wfagpu.Span(0, 0, 50, 50)
    cfg = lib.wfagpu_amd_configure_affine2p_span
    for sym in ("wfagpu_amd_align_device_2p_span", "wfagpu_amd_configure_affine2p_span"):
        assert sym in wfagpu.ABI_SYMBOLS and hasattr(lib, sym)
    try:
        assert cfg(C.byref(pen), C.byref(span)) == 0
        for bad in (wfagpu.Span(-1, 0, 0, 0), wfagpu.Span(0, 0, 0, -5)):
            assert cfg(C.byref(pen), C.byref(bad)) == -1
        assert cfg(C.byref(wfagpu.Penalties2p(4, 6, 0, 24, 1)), C.byref(span)) == -1
        # still configured: the others are refused as under two pieces alone
        assert lib.wfagpu_amd_configure_span(C.byref(span)) == -1
        assert lib.wfagpu_amd_configure_linear(C.byref(wfagpu.Linear(1, 0, 0))) == -1
        assert lib.wfagpu_amd_configure_wfadaptive(C.byref(wfagpu.WfAdaptive(10, 50, 1))) == -1
        assert cfg(C.byref(pen), None) == 0 and cfg(None, C.byref(span)) == 0      # (end to end; cleared)
        # refused, state left alone, while a gap-affine span, a metric or the heuristic is configured
        for setter, arg in ((lib.wfagpu_amd_configure_span, span), (lib.wfagpu_amd_configure_linear, wfagpu.Linear(1, 0, 0)),
                            (lib.wfagpu_amd_configure_wfadaptive, wfagpu.WfAdaptive(10, 50, 1))):
            assert setter(C.byref(arg)) == 0
            assert cfg(C.byref(pen), C.byref(span)) == -1
            assert setter(None) == 0
        wfagpu.configure_affine2p((4, 6, 2, 24, 1), span=(0, 0, 50, 50))
        assert lib.wfagpu_amd_configure_affine2p(None) == 0      # (clears both)
        assert lib.wfagpu_amd_configure_span(C.byref(span)) == 0
        with pytest.raises(ValueError):
            wfagpu.configure_affine2p((4, 6, 2, 24, 1), span=(0, 0, 50, 50))
    finally:
        lib.wfagpu_amd_configure_span(None)
        wfagpu.configure_affine2p()


P2 = ["--affine2p", "4,6,2,24,1"]


@pytest.mark.parametrize("args", [["--affine2p-ends-free", "0,0,5,5"], P2 + ["--affine2p-ends-free", "0,0,5"], P2 + ["--affine2p-ends-free", "0,0,5,5x"],
                                  P2 + ["--affine2p-ends-free", "0,-1,5,5"], P2 + ["--affine2p-ends-free", "0,0,5,5", "-B", "10"],
                                  ["-g", "2,3,1"] + P2 + ["--affine2p-ends-free", "0,0,5,5"], P2 + ["--affine2p-ends-free", "0,0,5,5", "--ends-free", "0,0,5,5"],
                                  P2 + ["--affine2p-ends-free", "0,0,5,5", "--metric-ends-free", "0,0,5,5"], P2 + ["--affine2p-ends-free", "0,0,5,5", "--edit"],
                                  P2 + ["--affine2p-ends-free", "0,0,5,5", "--wfa-adaptive", "10,50,1"], P2 + ["--ends-free", "0,0,5,5"]])
def test_cli_usage_errors_come_before_any_device_work(args, golden_dir):
    r = subprocess.run([CLI, "-i", os.path.join(golden_dir, "seq1k.seq")] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "--affine2p" in r.stderr and "ERROR" in r.stderr
    assert "HIP device" not in r.stderr and "Reading sequences" not in r.stdout + r.stderr
