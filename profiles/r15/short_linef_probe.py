"""Tier 5 under a metric with an ends-free span (short_kernel_linef.hip) against a build of the parent commit (the one-wave kernels of
align_kernel_linef.hip) and against the emulation a caller had (gap-affine (1,0,1) under the same span on the gap-affine ends-free kernels).

  python profiles/r15/short_linef_probe.py --parent-lib <libwfagpu.so of the parent commit> --out <dir>

The driver starts one child process per build, alternating: this build twice first (the spread of repeating the same build), then
parent / this build for --rounds rounds.  A child runs every workload, score-only and with CIGARs; the variants of a workload alternate
inside the child, medians of 7 calls after 2 warm-up calls each; DeviceAligner.stats() stage timers (wavefront kernel + backtrace).
  barcodes24_w32   1M 24-base barcodes (0-2 substitutions) somewhere in a 32-base window, span (0,0,8,8), edit, max_error 3: 32 lanes
  barcodes24_w40   the same in 40-base windows, span (0,0,16,16): 64 lanes
  reads150_w170_2pct / _5pct   100k 150-base reads (substitutions at that rate, one deleted base in every second read) somewhere in a
                   170-base window, span (0,0,20,20), edit, max_error 15: 64 lanes
  reads150_w170_2pct_lin32     the 2 % reads under ("linear", 3, 2), max_error 30 (the same 15 gap bases): 64 lanes"""
import argparse
import json
import os
import subprocess
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "wfa-gpu_amd", "bindings"))
REPS, WARM = 8, 2      # (the last call of the eight fetches the results and is not timed)


def in_windows(wfagpu, n, plen, wlen, sub_rate, delete_every, seed):
    """n pairs at a fixed stride: a random pattern of plen bases; the text is a window of wlen random bases with the pattern, damaged,
    written at a random offset of 0 .. wlen - plen (sub_rate: substitutions per base; delete_every: one base deleted in every such pair)."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    pat = rng.integers(0, 4, size=(n, plen))
    txt = rng.integers(0, 4, size=(n, wlen))
    dmg = np.where(rng.random((n, plen)) < sub_rate, (pat + rng.integers(1, 4, size=(n, plen))) % 4, pat)
    if delete_every:
        cut = np.arange(n) % delete_every == 0
        dmg[cut, plen // 2:-1] = dmg[cut, plen // 2 + 1:]
        dmg[cut, -1] = rng.integers(0, 4, size=int(cut.sum()))
    off = rng.integers(0, wlen - plen + 1, size=n)
    cols = off[:, None] + np.arange(plen)[None, :]
    txt[np.arange(n)[:, None], cols] = dmg
    ps, ts = (plen + 4) & ~3, (wlen + 4) & ~3
    buf = np.zeros((n, ps + ts), dtype=np.uint8)
    buf[:, :plen] = acgt[pat]
    buf[:, ps:ps + wlen] = acgt[txt]
    meta = np.zeros(n, dtype=wfagpu.META_DTYPE)
    meta["pattern_offset"] = np.arange(n, dtype=np.uint64) * (ps + ts)
    meta["text_offset"] = meta["pattern_offset"] + ps
    meta["pattern_len"] = plen
    meta["text_len"] = wlen
    return np.concatenate([buf.reshape(-1), np.zeros(16, dtype=np.uint8)]), meta


def child(lib_path):
    import wfagpu
    if lib_path:
        wfagpu.LIB_PATH = lib_path
    al = wfagpu.DeviceAligner(0)
    al_emu = wfagpu.DeviceAligner(0, no_auto_budget=1)
    r2 = in_windows(wfagpu, 100_000, 150, 170, 0.02, 2, 20261202)
    work = [("barcodes24_w32", in_windows(wfagpu, 1_000_000, 24, 32, 0.04, 0, 20261201), (0, 0, 8, 8), ("edit",), 3),
            ("barcodes24_w40", in_windows(wfagpu, 1_000_000, 24, 40, 0.04, 0, 20261203), (0, 0, 16, 16), ("edit",), 3),
            ("reads150_w170_2pct", r2, (0, 0, 20, 20), ("edit",), 15),
            ("reads150_w170_5pct", in_windows(wfagpu, 100_000, 150, 170, 0.05, 2, 20261205), (0, 0, 20, 20), ("edit",), 15),
            ("reads150_w170_2pct_lin32", r2, (0, 0, 20, 20), ("linear", 3, 2), 30)]
    for name, (buf, meta), span, metric, max_error in work:
        batches = {"metric": (al, al.upload(buf, meta), None, metric)}
        if metric == ("edit",):
            batches["emulation"] = (al_emu, al_emu.upload(buf, meta), (1, 0, 1), None)
        for cigar in (False, True):
            times, res, stats = {k: [] for k in batches}, {}, {}
            for rep in range(WARM + REPS):
                for k, (a, batch, pen, lin) in batches.items():
                    last = rep == WARM + REPS - 1      # (results come to the host once: a million CIGAR strings take longer than the call)
                    s, c = a.align(batch, pen, max_error=max_error, compute_cigar=cigar, linear=lin, span=span, fetch=last)
                    st = a.stats()
                    if rep >= WARM and not last:
                        times[k].append((st.align_ms, st.trace_ms))
                    if last:
                        res[k] = (int(s.astype(np.int64).sum()), zlib.crc32(s.astype(np.int32).tobytes()), zlib.crc32("\n".join(c).encode()) if cigar else 0)
                    stats[k] = {"pairs_tier": list(st.pairs_tier), "pairs_retried": st.pairs_retried, "main_launch_tier": st.main_launch_tier, "lanes_or_wpe": st.waves_per_simd_tier0}
            out = {"workload": name, "cigar": cigar}
            for k in batches:
                a = np.median(np.array(times[k]), axis=0)
                out[k] = {"align_ms": round(float(a[0]), 4), "trace_ms": round(float(a[1]), 4), "score_sum": res[k][0], "score_crc": res[k][1], "cigar_crc": res[k][2], **stats[k]}
            print("RESULT " + json.dumps(out), flush=True)
    for a in (al, al_emu):
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
        with open(os.path.join(a.out, "short_linef_probe.json"), "w") as f:
            json.dump(runs, f, indent=1)
    # the table: per workload and variant, every run's align_ms + trace_ms; results must be the same everywhere
    lines = []
    for w, row0 in enumerate(runs[0]["rows"]):
        lines.append(f"{row0['workload']} {'cigar' if row0['cigar'] else 'score'}")
        for k in ("metric", "emulation"):
            if k not in row0:
                continue
            for build in ("this", "parent"):
                sel = [r["rows"][w][k] for r in runs if r["build"] == build]
                if sel:
                    ms = " ".join("%.4f" % (v["align_ms"] + v["trace_ms"]) for v in sel)
                    lines.append(f"  {k:9s} {build:6s} align+trace ms per run: {ms}   "
                                 f"pairs_tier {sel[0]['pairs_tier']} lanes/wpe {sel[0]['lanes_or_wpe']} retried {sel[0]['pairs_retried']}")
            same = {(r["rows"][w][k]["score_crc"], r["rows"][w][k]["cigar_crc"]) for r in runs}
            lines.append(f"  {k:9s} scores and CIGAR bytes identical over all runs and builds: {len(same) == 1}")
        if "emulation" in row0:
            both = {r["rows"][w][k]["score_crc"] for r in runs for k in ("metric", "emulation")}
            lines.append(f"  metric == emulation (scores): {len(both) == 1}")
    with open(os.path.join(a.out, "short_linef_probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
