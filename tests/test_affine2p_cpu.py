"""Two-piece gap-affine alignment without a GPU: the golden files against an independent dynamic program and (where the reference is
compiled in place) against WFA2 run live; the CIGAR checker; the host-side pieces -- the new symbols, wfagpu_amd_configure_affine2p,
the -c verification under two pieces, the command line's usage errors."""
import ctypes as C
import hashlib
import math
import os
import subprocess

import numpy as np
import pytest

import affine2p_ref as a2
import oracle_lib
import wfagpu

PKG = os.path.dirname(wfagpu.LIB_PATH)
CLI = os.path.join(PKG, "bin", "wfa.affine.gpu")
ALL_SETS = a2.SETS + (a2.ONE_PEN_SET,)
CIGAR_SETS = ALL_SETS + (a2.LONG_SET,)      # (what does not go through the dynamic program: minutes on 33 kbp)
PAIRS_SHA1 = "cd206f15e1a8941031ee00a0b26883babd908449"      # of the pairs of small, gaps and ties as make_set builds them


@pytest.fixture(scope="module")
def sets():
    return {name: a2.read_golden(name) for name in CIGAR_SETS + (a2.SWEEP_SET,)}


def test_golden_sets_have_the_shapes_they_are_for(sets):
    small, gaps, ties = sets["small"], sets["gaps"], sets["ties"]
    assert len(small["pairs"]) == 400 and len(gaps["pairs"]) == 48 and len(ties["pairs"]) == 32
    assert any(len(p) == 0 for p, _ in small["pairs"]) and any(len(t) == 0 for _, t in small["pairs"])
    assert any(p == t and len(p) > 0 for p, t in small["pairs"])
    assert max(max(len(p), len(t)) for p, t in small["pairs"]) <= 300
    assert 8 <= sum(1 for p, t in small["pairs"] if set(p + t) - set(b"ACGT")) <= 16
    assert set(small["pens"]) == set(a2.PENS) and set(gaps["pens"]) == set(a2.PENS)
    assert set(sets[a2.ONE_PEN_SET]["pens"]) == {a2.DEFAULT_PEN} and sets[a2.ONE_PEN_SET]["pairs"] == small["pairs"]
    assert all(1075 <= len(s) <= 1325 for pair in gaps["pairs"] for s in pair)
    # both pieces are used: some gap run of a golden CIGAR is cheaper under the first piece, some under the second
    first = second = 0
    for cg, pen in zip(gaps["cigars"], gaps["pens"]):
        for n, op in a2.parse_cigar(cg):
            if op in "ID" and a2.crossover(pen):
                first += pen[1] + n * pen[2] < pen[3] + n * pen[4]
                second += pen[1] + n * pen[2] > pen[3] + n * pen[4]
    assert first > 20 and second > 10
    # ties: a gap of exactly the crossover length (in the few pairs with noise next to the repeat it may merge with another one)
    exact = sum(any(op in "ID" and n == a2.crossover(pen) for n, op in a2.parse_cigar(cg)) for cg, pen in zip(ties["cigars"], ties["pens"]))
    assert exact >= 28
    assert all(len(p) > 32766 and len(t) > 32766 for p, t in sets[a2.LONG_SET]["pairs"])
    assert sum(os.path.getsize(a2.golden_path(name)) for name in CIGAR_SETS) < (1 << 20)
    # (the pairs are rebuilt, not stored: the recipe must give the same bytes everywhere)
    digest = hashlib.sha1(b"".join(p + b"|" + t + b"\n" for name in a2.SETS for p, t in sets[name]["pairs"])).hexdigest()
    assert digest == PAIRS_SHA1


def test_the_sweep_has_the_shape_it_is_for(sets):
    """11 penalty sets of 20 short pairs each and 5 long pairs under M rings of 64 and 66 rows; every set has its byte-compare pair and its
    empty side; a deep ring gets short pairs (endsfree_ref.sweep_top).  The shapes of the second piece the sets are for are checked on
    the golden CIGARs: where it always wins every gap run is priced by it, where it never does none is."""
    g = sets[a2.SWEEP_SET]
    groups = a2.groups(g)
    assert len(g["pairs"]) == 11 * 20 + 2 * 5 and set(groups) == set(a2.SWEEP_PENS) and len(a2.SWEEP_PENS) == 11
    assert sorted(a2.ring_depth(pen) for pen in a2.SWEEP_PENS)[-3:] == [64, 65, 66] and [a2.ring_depth(pen) for pen in a2.SWEEP_LONG_PENS] == [64, 66]
    assert sum(1 for pen in a2.SWEEP_PENS if math.gcd(*pen) > 1) == 1
    for pen, idx in groups.items():
        short = [g["pairs"][i] for i in idx[:20]]
        assert len(idx) == (25 if pen in a2.SWEEP_LONG_PENS else 20)
        assert all(600 <= len(p) <= 800 and 600 <= len(t) <= 800 for p, t in (g["pairs"][i] for i in idx[20:]))
        assert sum(1 for p, t in short if set(p + t) - set(b"ACGT")) == 1 and sum(1 for p, t in short if not p or not t) == 1
        assert max(max(len(p), len(t)) for p, t in short) <= (48 if a2.ring_depth(pen) >= 60 else 160)
    runs = lambda pen: [n for i in groups[pen] for n, op in a2.parse_cigar(g["cigars"][i]) if op in "ID"]
    second = lambda pen, n: pen[3] + n * pen[4] < pen[1] + n * pen[2]
    assert len(runs((4, 6, 2, 3, 1))) > 20 and all(second((4, 6, 2, 3, 1), n) for n in runs((4, 6, 2, 3, 1)))
    assert len(runs((2, 1, 1, 1, 3))) > 20 and not any(second((2, 1, 1, 1, 3), n) for n in runs((2, 1, 1, 1, 3)))
    for pen in ((4, 24, 1, 6, 2), (5, 2, 6, 20, 5), (3, 2, 3, 9, 1)):      # both pieces are used
        assert any(second(pen, n) for n in runs(pen)) and not all(second(pen, n) for n in runs(pen)), pen
    assert any(not p for p, _ in g["pairs"]) and any(not t for _, t in g["pairs"])
    assert os.path.getsize(a2.golden_path(a2.SWEEP_SET)) < (64 << 10)


@pytest.mark.parametrize("name", ALL_SETS + (a2.SWEEP_SET,))
def test_golden_scores_equal_the_dynamic_program(sets, name):
    g = sets[name]
    for i, ((p, t), pen) in enumerate(zip(g["pairs"], g["pens"])):
        assert a2.dp_affine2p_score(p, t, pen) == g["scores"][i], (name, i, pen)


@pytest.mark.parametrize("name", CIGAR_SETS + (a2.SWEEP_SET,))
def test_golden_cigars_are_valid_and_cost_their_score(sets, name):
    g = sets[name]
    for i, ((p, t), pen) in enumerate(zip(g["pairs"], g["pens"])):
        ok, cost = a2.check_cigar2p(p, t, g["cigars"][i], pen)
        assert ok and cost == g["scores"][i], (name, i, pen, g["cigars"][i])


def test_cigar_checker_prices_by_the_cheaper_piece_and_refuses_what_is_wrong():
    pen = (4, 6, 2, 24, 1)
    p = b"ACGTACGTAC" + b"G" * 30 + b"TTGACCA"
    t = b"ACGTACGTAC" + b"G" * 10 + b"TTGACCA"
    assert a2.check_cigar2p(p, t, "10M20D17M", pen) == (True, 24 + 20)          # the second piece: 44 < 46
    assert a2.check_cigar2p(p, t, "20M20D7M", pen) == (True, 44)
    assert a2.check_cigar2p(p[:-1] + b"T", t, "10M20D16M1X", pen) == (True, 48)
    assert a2.check_cigar2p(b"ACGT", b"ACT", "2M1D1M", pen) == (True, 8)            # the first piece: 8 < 25
    assert not a2.check_cigar2p(p, t, "10M20D16M1X", pen)[0]                        # X on a match
    assert not a2.check_cigar2p(p, t, "10M10D10D17M", pen)[0]                       # equal neighbours
    assert not a2.check_cigar2p(p, t, "10M19D17M", pen)[0]                          # does not cover the pattern
    assert a2.check_cigar2p(p, t, "10M21D17M", pen) == (False, -1)                  # runs past the pattern


@pytest.mark.skipif(not oracle_lib.have_ref(), reason="the reference's WFA2 is not compiled in place here")
@pytest.mark.parametrize("name", CIGAR_SETS + (a2.SWEEP_SET,))
def test_wfa2_run_live_equals_the_golden_files(sets, name):
    g = sets[name]
    scores, cigars = a2.wfa2_affine2p(g["pairs"], g["pens"])
    assert np.array_equal(scores, g["scores"]) and cigars == g["cigars"], name


@pytest.mark.skipif(not oracle_lib.have_ref(), reason="the reference's WFA2 is not compiled in place here")
def test_wfa2_with_equal_pieces_agrees_with_its_gap_affine_self(golden_dir):
    """(x, o, e, o, e) against gap-affine (x, o, e) in WFA2 itself, on the reference's 1 kbp pairs: what the GPU test of equal pieces
    relies on."""
    pairs = wfagpu.read_seq_file(os.path.join(golden_dir, "seq1k.seq"))[:64]
    buf, meta = wfagpu.layout_pairs(pairs)
    for x, o, e in ((2, 3, 1), (5, 3, 2)):
        s2, c2 = a2.wfa2_affine2p(pairs, [(x, o, e, o, e)] * len(pairs))
        s1, c1, _ = oracle_lib.oracle_batch(buf, meta, (x, o, e), cigar=True)
        assert np.array_equal(s2, s1) and c2 == c1


def test_new_symbols_and_the_penalties_struct():
    lib = wfagpu.load()
    for sym in ("wfagpu_amd_align_device_2p", "wfagpu_amd_configure_affine2p"):
        assert sym in wfagpu.ABI_SYMBOLS and hasattr(lib, sym)
    assert C.sizeof(wfagpu.Penalties2p) == 5 * C.sizeof(C.c_int)
    assert [f for f, _ in wfagpu.Penalties2p._fields_] == ["mismatch", "gap_opening1", "gap_extension1", "gap_opening2", "gap_extension2"]
    header = open(os.path.join(os.path.dirname(PKG), "include", "wfa_gpu_device.h")).read()
    assert "typedef struct { int mismatch, gap_opening1, gap_extension1, gap_opening2, gap_extension2; } wfagpu_amd_penalties2p_t;" in header


def test_configure_affine2p_rejects_what_wfa2_rejects_and_leaves_the_state_alone():
    lib = wfagpu.load()
    try:
        assert lib.wfagpu_amd_configure_affine2p(C.byref(wfagpu.Penalties2p(4, 6, 2, 24, 1))) == 0
        for bad in ((0, 6, 2, 24, 1), (4, 0, 2, 24, 1), (4, 6, 0, 24, 1), (4, 6, 2, -24, 1), (4, 6, 2, 24, 0)):
            assert lib.wfagpu_amd_configure_affine2p(C.byref(wfagpu.Penalties2p(*bad))) == -1
        # still configured: a span is refused while it is
        assert lib.wfagpu_amd_configure_span(C.byref(wfagpu.Span(0, 0, 5, 5))) == -1
        assert lib.wfagpu_amd_configure_affine2p(None) == 0
        # and the other way round
        assert lib.wfagpu_amd_configure_span(C.byref(wfagpu.Span(0, 0, 5, 5))) == 0
        assert lib.wfagpu_amd_configure_affine2p(C.byref(wfagpu.Penalties2p(4, 6, 2, 24, 1))) == -1
        assert lib.wfagpu_amd_configure_span(None) == 0
        with pytest.raises(ValueError):
            wfagpu.configure_affine2p((4, 6, 2, 24, -1))
        wfagpu.configure_affine2p((2, 4, 2, 12, 1))
    finally:
        wfagpu.configure_affine2p()
        wfagpu.configure_span()


def test_verification_under_two_pieces(sets):
    """The CPU side of the command line's -c: the five-table scorer equals the dynamic program on small, the CIGAR is priced by the
    cheaper piece per gap run."""
    lib = wfagpu.load()
    lib.verification_cpu_score_2p.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t] + [C.c_int] * 5
    lib.verification_cpu_score_2p.restype = C.c_int
    lib.check_affine2p_distance.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_int] + [C.c_int] * 5 + [C.c_char_p]
    lib.check_affine2p_distance.restype = C.c_bool
    lib.check_cigar_edit.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_char_p]
    lib.check_cigar_edit.restype = C.c_bool
    for name in ("small", "ties"):
        g = sets[name]
        for i, ((p, t), pen) in enumerate(zip(g["pairs"], g["pens"])):
            want = a2.dp_affine2p_score(p, t, pen)
            assert lib.verification_cpu_score_2p(p, t, len(p), len(t), *pen) == want, (name, i, pen)
            cg = g["cigars"][i].encode()
            assert lib.check_cigar_edit(t, p, len(t), len(p), cg)
            assert lib.check_affine2p_distance(t, p, len(t), len(p), int(want), *pen, cg), (name, i, pen)
            assert not lib.check_affine2p_distance(t, p, len(t), len(p), int(want) + 1, *pen, cg)


@pytest.mark.parametrize("args", [["--affine2p", "4,6,2,24"], ["--affine2p", "4,6,2,24,0"], ["--affine2p", "4,6,2,24,1x"],
                                  ["--affine2p", "4,-6,2,24,1"], ["--affine2p", "4,6,2,24,1", "-g", "2,3,1"],
                                  ["--affine2p", "4,6,2,24,1", "-B", "10"], ["--affine2p", "4,6,2,24,1", "--ends-free", "0,0,5,5"]])
def test_cli_usage_errors_come_before_any_device_work(args, golden_dir):
    seq = os.path.join(golden_dir, "seq1k.seq")
    r = subprocess.run([CLI, "-i", seq] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "--affine2p" in r.stderr and "ERROR" in r.stderr
    assert "HIP device" not in r.stderr and "Reading sequences" not in r.stdout + r.stderr
