"""`bench.py --dump-outputs DIR`: the arrays of the last timed step as .npy files, the same from run to run, and a plain run
(no --full) that carries the headline figures without the checker's legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import oracle_lib
import wfagpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _text_rows(d):
    rows = np.load(os.path.join(d, "cigar_sample_text.npy"))
    assert rows.dtype == np.float32
    return [bytes(rows[r][rows[r] > 0].astype(np.uint8)).decode() for r in range(len(rows))]


def test_write_outputs_layout_sampling_and_size_bound(tmp_path, monkeypatch):
    """Per-pair values whole, CIGAR texts for a seeded sample that is the same on every call and shrinks to the byte budget."""
    n = 6000
    rng = np.random.default_rng(3)
    scores = rng.integers(0, 300, n).astype(np.int32)
    cigars = [b"%dM%dX" % (i + 1, int(s)) if i % 97 else b"" for i, s in enumerate(scores)]
    lens = [len(c) if i % 97 else -1 for i, c in enumerate(cigars)]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.write_outputs(a, scores, lens, lambda i: cigars[i])
    bench.write_outputs(b, scores, lens, lambda i: cigars[i])
    assert sorted(os.listdir(a)) == ["cigar_lengths.npy", "cigar_sample_index.npy", "cigar_sample_text.npy", "scores.npy"]
    for f in os.listdir(a):
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y)
    assert np.array_equal(np.load(os.path.join(a, "scores.npy")), scores.astype(np.float64))
    assert np.array_equal(np.load(os.path.join(a, "cigar_lengths.npy")), np.asarray(lens, dtype=np.float64))
    idx = np.load(os.path.join(a, "cigar_sample_index.npy")).astype(int)
    assert len(idx) == 4096 and len(set(idx)) == 4096 and (np.diff(idx) > 0).all()
    assert _text_rows(a) == [cigars[i].decode() for i in idx]
    # a text budget of 1000 bytes: 250 float32 values, rows as wide as the longest sampled CIGAR
    monkeypatch.setattr(bench, "DUMP_TEXT_BYTES", 1000)
    c = str(tmp_path / "c")
    bench.write_outputs(c, scores, lens, lambda i: cigars[i])
    small = np.load(os.path.join(c, "cigar_sample_text.npy"))
    few = np.load(os.path.join(c, "cigar_sample_index.npy")).astype(int)
    assert 0 < small.size * 4 <= 1000 and len(few) == len(small) and set(few) <= set(idx)
    assert _text_rows(c) == [cigars[i].decode() for i in few]
    # more pairs than are written whole: a seeded sample of them, with its index
    monkeypatch.setattr(bench, "DUMP_ALL_PAIRS", 1000)
    d = str(tmp_path / "d")
    bench.write_outputs(d, scores, rank=1, world=2)
    keep = np.load(os.path.join(d, "pair_index.rank1.npy")).astype(int)
    assert len(keep) == 1000 and (np.diff(keep) > 0).all()
    assert np.array_equal(np.load(os.path.join(d, "scores.rank1.npy")), scores[keep].astype(np.float64))
    assert sorted(os.listdir(d)) == ["pair_index.rank1.npy", "scores.rank1.npy"]


@pytest.mark.gpu
def test_plain_bench_run_dumps_the_last_steps_outputs(tmp_path):
    """A plain run of the flagship workload's kernels on 3000 pairs: the line carries the contract's fields and none of the --full
    legs, --steps sets the timed steps, and the dumped scores and CIGAR strings are the checker's for the same seeded pairs."""
    n, out_dir = 3000, str(tmp_path / "out")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--pairs", str(n),
                        "--dump-outputs", out_dir], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["metric"] == "alignments_per_sec" and line["unit"] == "alignments/s" and line["higher_is_better"] is True
    assert line["dtype"] == "int32" and line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert abs(line["value"] - n / (line["ms_per_step"] * 1e-3)) <= 0.01 * line["value"]
    for key in ("parity_sample", "host_to_host", "cpu_baseline", "configs", "cli_wall", "ont_banded"):
        assert key not in line
    wl = bench.WORKLOADS["cfg3"]
    buf, meta = wfagpu.generate_pairs(n, wl["length"], wl["error"], seed=1000)
    s_ref, c_ref, _ = oracle_lib.oracle_batch(buf, meta, bench.PEN, cigar=True, nthreads=8)
    assert np.array_equal(np.load(os.path.join(out_dir, "scores.npy")), s_ref.astype(np.float64))
    assert np.array_equal(np.load(os.path.join(out_dir, "cigar_lengths.npy")), np.array([len(c) for c in c_ref], dtype=np.float64))
    idx = np.load(os.path.join(out_dir, "cigar_sample_index.npy")).astype(int)
    assert len(idx) == n and _text_rows(out_dir) == [c_ref[i] for i in idx]
    assert sum(os.path.getsize(os.path.join(out_dir, f)) for f in os.listdir(out_dir)) < 64e6
