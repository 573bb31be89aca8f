"""Tier 5 under two-piece penalties (short_kernel_2p.hip) against a build of the parent commit (the one-wave kernels of
align_kernel_2p.hip), and its two group widths against each other.

  python profiles/r19/short_2p_probe.py --parent-lib <libwfagpu.so of the parent commit> --out <dir>

The driver starts one child process per build, alternating: this build twice first (the spread of repeating the same build), then
parent / this build for --rounds rounds.  A child runs 100k generated 150-base pairs at 2 % and at 5 % error under (4,6,2,24,1) with
max_error 30 (16 lanes) and 52 (32 lanes), score-only and with CIGARs; medians of 7 calls after 2 warm-up calls; DeviceAligner.stats()
stage timers (wavefront kernels + backtrace).  Variants: "planned" -- the lanes plan_tier picks; "wider" -- 32 lanes forced on the
16-lane calls (tuning.waves_per_simd, this build only); "affine" -- gap-affine (4,6,2) under the same budget, for context.
"untouched": 10k pairs of 1 kbp at 5 % under max_error 400, a two-piece call the tier does not take."""
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
PEN = (4, 6, 2, 24, 1)


def child(lib_path, parent):
    import wfagpu
    if lib_path:
        wfagpu.LIB_PATH = lib_path
    al = wfagpu.DeviceAligner(0)
    wide = None if parent else wfagpu.DeviceAligner(0, waves_per_simd=32)
    work = [("reads150_2pct", wfagpu.generate_pairs(100_000, 150, 0.02, seed=20261901), (30, 52)),
            ("reads150_5pct", wfagpu.generate_pairs(100_000, 150, 0.05, seed=20261902), (30, 52)),
            ("untouched_1kbp_5pct", wfagpu.generate_pairs(10_000, 1000, 0.05, seed=20261903), (400,))]
    for name, (buf, meta), budgets in work:
        for max_error in budgets:
            calls = {"planned": (al, al.upload(buf, meta), {"affine2p": PEN}, None)}
            if max_error <= 52:
                calls["affine"] = (al, calls["planned"][1], {}, PEN[:3])
            if wide is not None and max_error == 30:
                calls["wider"] = (wide, wide.upload(buf, meta), {"affine2p": PEN}, None)
            for cigar in (False, True):
                times, res, stats = {k: [] for k in calls}, {}, {}
                for rep in range(WARM + REPS):
                    for k, (a, batch, kw, pen) in calls.items():
                        last = rep == WARM + REPS - 1
                        s, c = a.align(batch, pen, max_error=max_error, compute_cigar=cigar, fetch=last, **kw)
                        st = a.stats()
                        if rep >= WARM and not last:
                            times[k].append((st.align_ms, st.trace_ms))
                        if last:
                            res[k] = (zlib.crc32(s.astype(np.int32).tobytes()), zlib.crc32("\n".join(c).encode()) if cigar else 0)
                        stats[k] = {"pairs_tier": list(st.pairs_tier), "pairs_retried": st.pairs_retried, "main_launch_tier": st.main_launch_tier, "lanes_or_wpe": st.waves_per_simd_tier0}
                out = {"workload": "%s e%d" % (name, max_error), "cigar": cigar}
                for k in calls:
                    a = np.median(np.array(times[k]), axis=0)
                    out[k] = {"align_ms": round(float(a[0]), 4), "trace_ms": round(float(a[1]), 4), "score_crc": res[k][0], "cigar_crc": res[k][1], **stats[k]}
                print("RESULT " + json.dumps(out), flush=True)
    for a in [al] + ([wide] if wide else []):
        a.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib", default="")
    ap.add_argument("--parent", action="store_true")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    if a.child:
        return child(a.lib, a.parent)
    order = ["this", "this"] + ["parent", "this"] * a.rounds if a.parent_lib else ["this", "this"]
    runs = []
    for i, build in enumerate(order):
        cmd = [sys.executable, os.path.abspath(__file__), "--child"] + (["--lib", os.path.abspath(a.parent_lib), "--parent"] if build == "parent" else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
        if r.returncode != 0:
            sys.exit(f"child {i} ({build}) ended with {r.returncode}: {r.stderr[-2000:]}")
        runs.append({"build": build, "rows": [json.loads(line[7:]) for line in r.stdout.splitlines() if line.startswith("RESULT ")]})
        print(i, build, "ok", flush=True)
    # the table: per workload and variant, every run's align_ms + trace_ms; "planned" must give the same results in every run and build
    lines = []
    for w, row0 in enumerate(runs[0]["rows"]):
        lines.append(f"{row0['workload']} {'cigar' if row0['cigar'] else 'score'}")
        for k in ("planned", "wider", "affine"):
            for build in ("this", "parent"):
                sel = [r["rows"][w][k] for r in runs if r["build"] == build and k in r["rows"][w]]
                if sel:
                    ms = " ".join("%.4f" % (v["align_ms"] + v["trace_ms"]) for v in sel)
                    lines.append(f"  {k:7s} {build:6s} align+trace ms per run: {ms}   "
                                 f"pairs_tier {sel[0]['pairs_tier']} lanes/wpe {sel[0]['lanes_or_wpe']} retried {sel[0]['pairs_retried']}")
        same = {(r["rows"][w][k]["score_crc"], r["rows"][w][k]["cigar_crc"]) for r in runs for k in ("planned", "wider") if k in r["rows"][w]}
        lines.append(f"  two-piece scores and CIGAR bytes identical over all runs, builds and widths: {len(same) == 1}")
    with open(os.path.join(a.out, "short_2p_probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
