#!/usr/bin/env python3
"""Kernel time per 1e9 rays of the aperture map (sart_trace_histogram_aperture_device) against the generic histogram entry with
spectra, the per-shell entry and the origin entry on the same box, the same rays and full-size tables (1968 x 1500):
    python tools/aperture_rate.py [rays] [repeats] [sides, comma-separated: default 256,1024]

BabyIAXO / XMM, f64 and FIXED64, image 256 x 256 with spectra (10 000 radial bins).  Per case, the median and the spread (max - min)
of `repeats` warm runs between two HIP events (launch + folds):
  hist generic    the histogram entry with SART_FORCE_GENERIC (the generic variant, which the breakdown kernels are built on)
  shells          the per-shell entry
  origin          the origin entry: three global atomics per passed ray into a map of 94 MB
  aperture 256    the aperture entry, 256 x 256 cells over +-1.02 x the largest R1 (2 MB): the same three atomics
  aperture 1024   the same, 1024 x 1024 cells (32 MB)
(one row per side given; the code of the launch does not depend on the side, only where its atomics land does)
The yardstick of the aperture rows is the origin row of the same run: the same atomics into a map 3 to 47 times smaller, so their
median should not exceed origin's median plus origin's spread.  The last lines say whether it does."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from solaraxionraytracing_amd import _lib as L   # noqa: E402
import solaraxionraytracing_amd as sa   # noqa: E402

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 6
sides = [int(v) for v in (sys.argv[3] if len(sys.argv) > 3 else "256,1024").split(",")]
stream = torch.cuda.Stream()


def timed(fn):
    ms = []
    for r in range(repeats + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        if r:   # the first run warms up (and places the LDS tile)
            ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(max(ms) - min(ms))


def tracer(full, env):
    for k, v in env.items():
        os.environ[k] = v
    try:
        return sa.RayTracer(full)
    finally:
        for k in env:
            os.environ.pop(k, None)


def main():
    full = sa.initFullSetup()
    n_r, n_e = full.diffFluxCDFs.shape
    half = 1.02 * max(full.setup.all_r1[:full.setup.n_shells])
    results = {}
    labels = [("hist generic", {"SART_FORCE_GENERIC": "1"}, None), ("shells", {}, "shells"), ("origin", {}, "origin")]
    labels += [("aperture %d" % side, {}, side) for side in sides]
    for label, env, what in labels:
        with torch.cuda.stream(stream):
            rt = tracer(full, env)
            try:
                rt.set_stream(stream.cuda_stream)
                if isinstance(what, int):
                    rt.set_aperture_grid(what, what, -half, half, -half, half)
                for mode in ("f64", "fixed64"):
                    rt.set_accumulation_mode(mode)
                    p = rt.shells_params(n, seed=1, spectra=True)
                    n_acc = 256 * 256 + L.SART_ACC_COUNT + 2 * p.n_radial_bins + 3 * (n_e + 1)
                    acc = torch.zeros(n_acc, dtype=torch.float64, device="cuda")
                    if what == "shells":
                        blk = torch.zeros(rt.shell_block_len(True), dtype=torch.float64, device="cuda")
                        res = timed(lambda: rt.trace_shells_device(p, acc.data_ptr(), blk.data_ptr()))
                    elif what == "origin":
                        blk = torch.zeros(rt.origin_block_len(), dtype=torch.float64, device="cuda")
                        res = timed(lambda: rt.trace_origin_device(p, acc.data_ptr(), blk.data_ptr()))
                    elif isinstance(what, int):
                        blk = torch.zeros(rt.aperture_block_len(), dtype=torch.float64, device="cuda")
                        res = timed(lambda: rt.trace_aperture_device(p, acc.data_ptr(), blk.data_ptr()))
                    else:
                        res = timed(lambda: rt.trace_histogram_device(p, acc.data_ptr()))
                    results[(label, mode)] = tuple(v * 1e9 / n for v in res)
            finally:
                rt.close()
    print("babyiaxo_xmm, %d x %d tables, %d rays per launch, %d repeats; ms per 1e9 rays: median +- spread (ratio to hist generic); "
          "library %s" % (n_r, n_e, n, repeats, os.path.basename(L.LIBSART_PATH)))
    for mode in ("f64", "fixed64"):
        base = results[("hist generic", mode)][0]
        print("%-8s " % mode + "  ".join("%s %7.2f +- %.2f (%.2f x)" % ((label,) + results[(label, mode)] + (results[(label, mode)][0] / base,))
                                         for label, _, _ in labels), flush=True)
    for mode in ("f64", "fixed64"):
        o_med, o_spread = results[("origin", mode)]
        for label in ("aperture %d" % side for side in sides):
            med = results[(label, mode)][0]
            print("%-8s %-13s median %.2f %s origin's median + spread %.2f" % (mode, label, med, "<=" if med <= o_med + o_spread else "ABOVE",
                                                                              o_med + o_spread), flush=True)


main()
