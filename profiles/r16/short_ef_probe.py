"""Tier 5 for gap-affine alignment under an ends-free span (short_kernel_ef*.hip) against a build of the parent commit (the one-wave
kernels of align_kernel_ef.hip), and its group widths against each other.

  python profiles/r16/short_ef_probe.py --parent-lib <libwfagpu.so of the parent commit> --out <dir>

The driver starts one child process per build, alternating: this build twice first (the spread of repeating the same build), then
parent / this build for --rounds rounds.  A child runs every workload under (2,3,1) and (5,3,2), score-only and with CIGARs; the variants
of a workload alternate inside the child, medians of 7 calls after 2 warm-up calls each; DeviceAligner.stats() stage timers (wavefront
kernel + backtrace).  Variant "planned": the lanes plan_tier picks; "wider": the next wider group forced through tuning.waves_per_simd
(this build only; planned 64: none).
  barcodes24_w28   1M 24-base barcodes (0-2 substitutions) somewhere in a 28-base window, span (0,0,4,4), max_error 6 / 10: 16 lanes
  barcodes24_w32   the same in 32-base windows, span (0,0,8,8): 32 lanes
  barcodes24_w40   the same in 40-base windows, span (0,0,16,16): 64 lanes
  reads150_w170_2pct / _5pct   100k 150-base reads (substitutions at that rate, one deleted base in every second read) somewhere in a
                   170-base window, span (0,0,20,20), max_error 24 / 48 -- the largest budgets whose bound fits 64 lanes"""
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


def child(lib_path, parent):
    import wfagpu
    if lib_path:
        wfagpu.LIB_PATH = lib_path
    al = wfagpu.DeviceAligner(0)
    wide = {} if parent else {32: wfagpu.DeviceAligner(0, waves_per_simd=32), 64: wfagpu.DeviceAligner(0, waves_per_simd=64)}
    # (name, pairs, span, max_error under (2,3,1) and under (5,3,2), planned lanes)
    work = [("barcodes24_w28", in_windows(wfagpu, 1_000_000, 24, 28, 0.04, 0, 20261211), (0, 0, 4, 4), (6, 10), 16),
            ("barcodes24_w32", in_windows(wfagpu, 1_000_000, 24, 32, 0.04, 0, 20261201), (0, 0, 8, 8), (6, 10), 32),
            ("barcodes24_w40", in_windows(wfagpu, 1_000_000, 24, 40, 0.04, 0, 20261203), (0, 0, 16, 16), (6, 10), 64),
            ("reads150_w170_2pct", in_windows(wfagpu, 100_000, 150, 170, 0.02, 2, 20261202), (0, 0, 20, 20), (24, 48), 64),
            ("reads150_w170_5pct", in_windows(wfagpu, 100_000, 150, 170, 0.05, 2, 20261205), (0, 0, 20, 20), (24, 48), 64)]
    for name, (buf, meta), span, budgets, lanes in work:
        batches = {"planned": (al, al.upload(buf, meta))}
        if 2 * lanes in wide:
            batches["wider"] = (wide[2 * lanes], wide[2 * lanes].upload(buf, meta))
        for pen, max_error in zip(((2, 3, 1), (5, 3, 2)), budgets):
            for cigar in (False, True):
                times, res, stats = {k: [] for k in batches}, {}, {}
                for rep in range(WARM + REPS):
                    for k, (a, batch) in batches.items():
                        last = rep == WARM + REPS - 1      # (results come to the host once: a million CIGAR strings take longer than the call)
                        s, c = a.align(batch, pen, max_error=max_error, compute_cigar=cigar, span=span, fetch=last)
                        st = a.stats()
                        if rep >= WARM and not last:
                            times[k].append((st.align_ms, st.trace_ms))
                        if last:
                            res[k] = (int(s.astype(np.int64).sum()), zlib.crc32(s.astype(np.int32).tobytes()), zlib.crc32("\n".join(c).encode()) if cigar else 0)
                        stats[k] = {"pairs_tier": list(st.pairs_tier), "pairs_retried": st.pairs_retried, "main_launch_tier": st.main_launch_tier, "lanes_or_wpe": st.waves_per_simd_tier0}
                out = {"workload": "%s x%do%de%d" % ((name,) + pen), "cigar": cigar}
                for k in batches:
                    a = np.median(np.array(times[k]), axis=0)
                    out[k] = {"align_ms": round(float(a[0]), 4), "trace_ms": round(float(a[1]), 4), "score_sum": res[k][0], "score_crc": res[k][1], "cigar_crc": res[k][2], **stats[k]}
                print("RESULT " + json.dumps(out), flush=True)
    for a in [al] + list(wide.values()):
        a.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib", default="")
    ap.add_argument("--parent", action="store_true")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.child:
        return child(a.lib, a.parent)
    order = ["this", "this"] + ["parent", "this"] * a.rounds if a.parent_lib else ["this", "this"]
    runs = []
    for i, build in enumerate(order):
        cmd = [sys.executable, os.path.abspath(__file__), "--child"] + (["--lib", os.path.abspath(a.parent_lib), "--parent"] if build == "parent" else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.exit(f"child {i} ({build}) ended with {r.returncode}: {r.stderr[-2000:]}")
        rows = [json.loads(line[7:]) for line in r.stdout.splitlines() if line.startswith("RESULT ")]
        runs.append({"run": i, "build": build, "rows": rows})
        print(i, build, "ok", flush=True)
        with open(os.path.join(a.out, "short_ef_probe.json"), "w") as f:
            f.write("[\n" + ",\n".join(json.dumps({"run": r["run"], "build": r["build"], **row}) for r in runs for row in r["rows"]) + "\n]\n")      # (a row per line)
    # the table: per workload and variant, every run's align_ms + trace_ms; results must be the same everywhere
    lines = []
    for w, row0 in enumerate(runs[0]["rows"]):
        lines.append(f"{row0['workload']} {'cigar' if row0['cigar'] else 'score'}")
        for k in ("planned", "wider"):
            for build in ("this", "parent"):
                sel = [r["rows"][w][k] for r in runs if r["build"] == build and k in r["rows"][w]]
                if sel:
                    ms = " ".join("%.4f" % (v["align_ms"] + v["trace_ms"]) for v in sel)
                    lines.append(f"  {k:7s} {build:6s} align+trace ms per run: {ms}   "
                                 f"pairs_tier {sel[0]['pairs_tier']} lanes/wpe {sel[0]['lanes_or_wpe']} retried {sel[0]['pairs_retried']}")
        same = {(r["rows"][w][k]["score_crc"], r["rows"][w][k]["cigar_crc"]) for r in runs for k in ("planned", "wider") if k in r["rows"][w]}
        lines.append(f"  scores and CIGAR bytes identical over all runs, builds and widths: {len(same) == 1}")
    with open(os.path.join(a.out, "short_ef_probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
