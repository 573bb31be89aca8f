#!/usr/bin/env python3
"""R10 probe: edit and gap-linear distance on the one-component kernels (align(..., linear=...)) against the emulation a caller had
before them, gap-affine with a zero opening on the existing kernels (align(batch, (x, 0, g))), on the same pairs, the same context, in
one process, the variants alternating.  100k x 1 kbp and 100k x 150 bp pairs at 5 % (wfagpu.generate_pairs, fixed seed), score-only and
with CIGARs, default and tuning.careful_only.  Prints min / median / max over REPS of stats.align_ms, trace_ms, total_ms, and cells.
The gap-affine kernels of this tree are instruction for instruction the parent commit's (profiles/r10/existing_kernels_unchanged.txt),
so the emulation's figures are the parent's."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "wfa-gpu_amd", "bindings"))
import wfagpu  # noqa: E402

REPS = 7
N = int(os.environ.get("PROBE_PAIRS", "100000"))


def main():
    for length, budget in ((1000, 150), (150, 40)):
        buf, meta = wfagpu.generate_pairs(N, length, 0.05, seed=20261021)
        for metric, pen, scale in ((("edit",), (1, 0, 1), 1), (("linear", 4, 2), (4, 0, 2), 4)):
            for cigar in (False, True):
                variants = []
                for careful in (0, 1):
                    variants.append((f"one-component {'careful_only' if careful else 'default'}", careful, dict(linear=metric), None))
                    variants.append((f"gap-affine {pen} {'careful_only' if careful else 'default'}", careful, {}, pen))
                als = {careful: wfagpu.DeviceAligner(0, careful_only=careful) for careful in (0, 1)}
                batches = {careful: als[careful].upload(buf, meta) for careful in (0, 1)}
                times = {v[0]: [] for v in variants}
                ref = None
                for rep in range(REPS + 1):      # (the first round warms every variant up and is not counted)
                    for name, careful, kw, p in variants:
                        al = als[careful]
                        s, c = al.align(batches[careful], p, max_error=budget * scale, compute_cigar=cigar, **kw)
                        st = al.stats()
                        if rep == 0:
                            if ref is None:
                                ref = (s.copy(), c)
                            else:
                                assert np.array_equal(s, ref[0]), name
                                assert c == ref[1], name
                        else:
                            times[name].append((st.align_ms, st.trace_ms, st.total_ms, st.cells))
                print(f"{N} x {length} bp @ 5 %, {metric}, max_error {budget * scale}, {'CIGARs' if cigar else 'score only'} (answers of the four variants equal)")
                for name, *_ in variants:
                    a = np.array(times[name], dtype=np.float64)
                    f = lambda col: f"{a[:, col].min():8.3f} {np.median(a[:, col]):8.3f} {a[:, col].max():8.3f}"
                    print(f"  {name:44s} align ms {f(0)} | trace ms {f(1)} | total ms {f(2)} | cells {int(a[0, 3])}")
                sys.stdout.flush()
                for al in als.values():
                    al.close()


if __name__ == "__main__":
    main()
