"""Tier 5 under the edit metric (short_kernel_lin.hip) against a build of the parent commit (the one-wave metric kernels) and against
the emulation a caller had (gap-affine (1,0,1) on gap-affine tier 5, same max_error, no budgets from a sample).

  python profiles/r14/short_lin_probe.py --parent-lib <libwfagpu.so of the parent commit> --out <dir>

The driver starts one child process per build, alternating: this build twice first (the spread of repeating the same build), then
parent / this build for three rounds.  A child runs every workload: 100k x 150 bp at 2 % and 5 % under max_error = 30, and 1M 24-base
barcodes against 24-30-base candidates under max_error = 3 and 6 (8-lane groups as planned, and 16-lane groups forced through
tuning.waves_per_simd = 16), score-only and with CIGARs; the variants of a workload alternate inside the child, medians of 7 calls
after 2 warm-up calls each; DeviceAligner.stats() stage timers and the host clock around the call."""
import argparse
import json
import os
import subprocess
import sys
import time
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "wfa-gpu_amd", "bindings"))
REPS, WARM = 8, 2      # (the last call of the eight fetches the results and is not timed)


def barcodes(wfagpu, n, seed):
    """n pairs: a 24-base barcode against a candidate of 24-30 bases -- half of them the barcode with 0-2 substitutions and 0-6 bases
    behind it, half unrelated --, laid out at a fixed stride of 64 bytes."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    bar = acgt[rng.integers(0, 4, size=(n, 24))]
    cand = acgt[rng.integers(0, 4, size=(n, 30))]
    related = np.arange(n) % 2 == 0
    cand[related, :24] = bar[related]
    for _ in range(2):
        hit = related & (rng.random(n) < 0.5)
        cand[hit, rng.integers(0, 24, size=int(hit.sum()))] = acgt[rng.integers(0, 4, size=int(hit.sum()))]
    tlen = 24 + rng.integers(0, 7, size=n)
    cand[np.arange(30)[None, :] >= tlen[:, None]] = 0
    buf = np.zeros((n, 64), dtype=np.uint8)
    buf[:, :24] = bar
    buf[:, 28:58] = cand
    meta = np.zeros(n, dtype=wfagpu.META_DTYPE)
    meta["pattern_offset"] = np.arange(n, dtype=np.uint64) * 64
    meta["text_offset"] = meta["pattern_offset"] + 28
    meta["pattern_len"] = 24
    meta["text_len"] = tlen
    return np.concatenate([buf.reshape(-1), np.zeros(16, dtype=np.uint8)]), meta


def child(lib_path):
    import wfagpu
    if lib_path:
        wfagpu.LIB_PATH = lib_path
    al = wfagpu.DeviceAligner(0)
    al16 = wfagpu.DeviceAligner(0, waves_per_simd=16)
    al_emu = wfagpu.DeviceAligner(0, no_auto_budget=1)
    work = [(f"reads150_{int(err * 100)}pct_e30", wfagpu.generate_pairs(100_000, 150, err, seed=20261126 + int(err * 100)), 30, False) for err in (0.02, 0.05)]
    bc = barcodes(wfagpu, 1_000_000, 20261127)
    work += [(f"barcodes24_e{me}", bc, me, True) for me in (3, 6)]
    for name, (buf, meta), max_error, with16 in work:
        batches = {"metric": (al, al.upload(buf, meta), None, ("edit",)), "emulation": (al_emu, al_emu.upload(buf, meta), (1, 0, 1), None)}
        if with16:
            batches["metric_l16"] = (al16, al16.upload(buf, meta), None, ("edit",))
        for cigar in (False, True):
            times, res, stats = {k: [] for k in batches}, {}, {}
            for rep in range(WARM + REPS):
                for k, (a, batch, pen, lin) in batches.items():
                    t0 = time.perf_counter()
                    last = rep == WARM + REPS - 1      # (results come to the host once: a million CIGAR strings take longer than the call)
                    s, c = a.align(batch, pen, max_error=max_error, compute_cigar=cigar, linear=lin, fetch=last)
                    wall = (time.perf_counter() - t0) * 1e3
                    st = a.stats()
                    if rep >= WARM and not last:
                        times[k].append((st.align_ms, st.trace_ms, st.total_ms, wall))
                    if last:
                        res[k] = (int(s.astype(np.int64).sum()), zlib.crc32("\n".join(c).encode()) if cigar else 0)
                    stats[k] = {"pairs_tier": list(st.pairs_tier), "pairs_retried": st.pairs_retried, "main_launch_tier": st.main_launch_tier, "lanes_or_wpe": st.waves_per_simd_tier0}
            out = {"workload": name, "cigar": cigar}
            for k in batches:
                a = np.median(np.array(times[k]), axis=0)
                out[k] = {"align_ms": round(float(a[0]), 4), "trace_ms": round(float(a[1]), 4), "total_ms": round(float(a[2]), 4), "wall_ms": round(float(a[3]), 4),
                          "score_sum": res[k][0], "cigar_crc": res[k][1], **stats[k]}
            print("RESULT " + json.dumps(out), flush=True)
    for a in (al, al16, al_emu):
        a.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib", default="")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.child:
        return child(a.lib)
    order = ["this", "this"] + ["parent", "this"] * a.rounds if a.parent_lib else ["this", "this"]
    runs = []
    for i, build in enumerate(order):
        cmd = [sys.executable, os.path.abspath(__file__), "--child"] + (["--lib", os.path.abspath(a.parent_lib)] if build == "parent" else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            sys.exit(f"child {i} ({build}) ended with {r.returncode}: {r.stderr[-2000:]}")
        rows = [json.loads(line[7:]) for line in r.stdout.splitlines() if line.startswith("RESULT ")]
        runs.append({"run": i, "build": build, "rows": rows})
        print(i, build, "ok", flush=True)
        with open(os.path.join(a.out, "short_lin_probe.json"), "w") as f:
            json.dump(runs, f, indent=1)
    # the table: per workload and variant, every run's align_ms + trace_ms; results must be the same everywhere
    lines = []
    first = runs[0]["rows"]
    for w, row0 in enumerate(first):
        lines.append(f"{row0['workload']} {'cigar' if row0['cigar'] else 'score'}")
        for k in ("metric", "metric_l16", "emulation"):
            if k not in row0:
                continue
            for build in ("this", "parent"):
                vals = [r["rows"][w][k]["align_ms"] + r["rows"][w][k]["trace_ms"] for r in runs if r["build"] == build]
                if vals:
                    tiers = [r["rows"][w][k]["pairs_tier"] for r in runs if r["build"] == build][0]
                    lines.append(f"  {k:11s} {build:6s} align+trace ms per run: {' '.join(f'{v:.4f}' for v in vals)}   pairs_tier {tiers}")
            same = {(r["rows"][w][k]["score_sum"], r["rows"][w][k]["cigar_crc"]) for r in runs}
            lines.append(f"  {k:11s} results identical over all runs and builds: {len(same) == 1}")
        both = {(r["rows"][w][k]["score_sum"], r["rows"][w][k]["cigar_crc"]) for r in runs for k in ("metric", "emulation")}
        lines.append(f"  metric == emulation (scores, CIGAR bytes): {len(both) == 1}")
    with open(os.path.join(a.out, "short_lin_probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
