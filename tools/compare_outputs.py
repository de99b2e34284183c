#!/usr/bin/env python3
"""Outputs of two builds, file for file (bench.py --dump-outputs DIR):

  python tools/compare_outputs.py --fixed64 PARENT_DIR NEW_DIR --f64-parent DIR [DIR ...] --f64-new DIR [DIR ...] [--json OUT]

FIXED64: image.npy and summary.npy must be byte-identical.  f64: the counters equal, the five per-lane sums compared to the last bit,
the largest pixel difference over the peak for every parent / parent pair (the parent's own scatter: the order of the f64 atomics
follows the timing) beside every parent / new pair."""
import argparse
import itertools
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from solaraxionraytracing_amd import _lib as L   # noqa: E402

SUMS = ("SUM_WEIGHTS", "SUM_WEIGHTS_SQ", "SUM_X", "SUM_Y", "SUM_R")


def load(d):
    return np.load(os.path.join(d, "image.npy")), np.load(os.path.join(d, "summary.npy"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fixed64", nargs=2, required=True)
    ap.add_argument("--f64-parent", nargs="+", required=True)
    ap.add_argument("--f64-new", nargs="+", required=True)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    (pi, ps), (ni, ns) = load(a.fixed64[0]), load(a.fixed64[1])
    out = {"fixed64_image_identical": pi.tobytes() == ni.tobytes(), "fixed64_summary_identical": ps.tobytes() == ns.tobytes()}
    par, new = [load(d) for d in a.f64_parent], [load(d) for d in a.f64_new]
    for key, slot in L.ACC.items():
        p, n = par[0][1][slot], new[0][1][slot]
        if key in SUMS:
            out["f64_" + key] = {"parent_vs_new_rel": float(abs(n - p) / abs(p)) if p else float(abs(n - p)),
                                 "bits_equal": bool(np.float64(p).view(np.uint64) == np.float64(n).view(np.uint64))}
        elif key.startswith("N_"):
            out["f64_%s_equal" % key] = bool(all(x[1][slot] == p for x in par + new))
    peak = float(par[0][0].max())
    diff = lambda x, y: float(np.abs(x[0] - y[0]).max() / peak)
    out["f64_image_max_abs_diff_over_peak_all_pairs"] = {
        "parent_runs": len(par), "new_runs": len(new),
        "parent_vs_parent": [diff(x, y) for x, y in itertools.combinations(par, 2)],
        "parent_vs_new": [diff(x, y) for x in par for y in new]}
    text = json.dumps(out, indent=1)
    print(text)
    if a.json:
        open(a.json, "w").write(text + "\n")
    return 0 if out["fixed64_image_identical"] and out["fixed64_summary_identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
