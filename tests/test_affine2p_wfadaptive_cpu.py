"""The wf-adaptive heuristic under two-piece penalties without a GPU: the golden files (tests/golden/affine2p_ad.*) hold valid CIGARs,
no score lies below the two-piece optimum, and the heuristic bites; the new symbols exist.
A golden CIGAR does not always cost its score under check_cigar2p: where the cut-off dropped the I2 / D2 cells of a long gap, WFA2's path
carries the gap on the first piece and WFA2 reports that path's score, while the printed run is priced by the cheaper piece.  So the
text costs the score or less (small: 11 of 200 pairs cost less, indel: 0 of 32, long: 0 of 4), never more, and never less than the optimum."""
import os
import subprocess

import pytest

import affine2p_ref as a2
import affine2p_wfadaptive_ref as ar
import wfagpu


CHEAPER = {"small": 11, "indel": 0, "long": 0}      # pairs whose text costs less than its score (the docstring above): pinned
CLI = os.path.join(os.path.dirname(wfagpu.LIB_PATH), "bin", "wfa.affine.gpu")


@pytest.mark.parametrize("name", ar.SETS)
def test_golden_cigars_are_valid_cost_their_score_and_never_beat_the_optimum(name):
    g = ar.read_golden(name)
    above = cheaper = 0
    for (p, t), pen, s, cg in zip(g["pairs"], g["pens"], g["scores"], g["cigars"]):
        valid, cost = a2.check_cigar2p(p, t, cg, pen)
        opt = a2.dp_affine2p_score(p, t, pen)
        assert valid and opt <= cost <= s, (len(p), len(t), pen, opt, cost, int(s))
        above += s > opt
        cheaper += cost < s
    assert above >= ar.MIN_ABOVE[name] and cheaper == CHEAPER[name]


def test_new_symbols():
    lib = wfagpu.load()
    for sym in ("wfagpu_amd_align_device_2p_adaptive", "wfagpu_amd_configure_affine2p_wfadaptive"):
        assert sym in wfagpu.ABI_SYMBOLS and hasattr(lib, sym)


P2, AD = ["--affine2p", "4,6,2,24,1"], ["--affine2p-wfa-adaptive", "10,50,1"]


@pytest.mark.parametrize("args", [P2 + AD + ["-B", "auto"], P2 + AD + ["--ends-free", "0,0,5,5"], P2 + AD + ["--affine2p-ends-free", "0,0,5,5"],
                                  P2 + AD + ["--wfa-adaptive", "10,50,1"], AD, P2 + [AD[0], "0,50,1"]])
def test_cli_usage_errors(tmp_path, args):
    """With -B, --ends-free, --affine2p-ends-free or --wfa-adaptive, without --affine2p, or with a bad member: a usage error before any
    device work (this test runs without a GPU)."""
    seq = tmp_path / "one.seq"
    seq.write_bytes(b">ACGT\n<ACGT\n")
    r = subprocess.run([CLI, "-i", str(seq)] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--affine2p-wfa-adaptive" in r.stderr, r.stderr[-500:]
