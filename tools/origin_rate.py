#!/usr/bin/env python3
"""Kernel time per 1e9 rays of the solar-origin map (sart_trace_histogram_origin_device) against the generic histogram entry with
spectra, the per-shell entry and the channel entry (T = 3) on the same box, the same rays and full-size tables (1968 x 1500: the
map is 8 + 1968 x 1500 x 4 slots, 94 MB):
    python tools/origin_rate.py [rays] [repeats]

BabyIAXO / XMM, f64 and FIXED64, image 256 x 256 with spectra (10 000 radial bins).  Per case, the median of `repeats` warm runs
between two HIP events (launch + folds):
  hist generic    the histogram entry with SART_FORCE_GENERIC (the generic variant, which the three breakdown kernels are built on)
  shells          the per-shell entry
  channels T=3    the channel entry, three channels of uniform random fractions (stride 4)
  origin          the origin entry: three global atomics per passed ray into the map
A library selected with SART_LIBSART that predates the origin entry (A/B timing of the untouched entries against an older build) is
timed without the origin row."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from solaraxionraytracing_amd import _lib as L

_probe = ctypes.CDLL(L.LIBSART_PATH)
HAS_ORIGIN = hasattr(_probe, "sart_trace_histogram_origin_device")
if not HAS_ORIGIN:
    for _name in [k for k in L.SART_SYMBOLS if "origin" in k]:
        del L.SART_SYMBOLS[_name]

import solaraxionraytracing_amd as sa   # noqa: E402

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 3
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
    return float(np.median(ms))


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
    results = {}
    labels = [("hist generic", {"SART_FORCE_GENERIC": "1"}, None), ("shells", {}, "shells"), ("channels T=3", {}, 3)]
    if HAS_ORIGIN:
        labels.append(("origin", {}, "origin"))
    for label, env, what in labels:
        with torch.cuda.stream(stream):
            rt = tracer(full, env)
            try:
                rt.set_stream(stream.cuda_stream)
                if isinstance(what, int):
                    gen = torch.Generator(device="cuda").manual_seed(5)
                    rates = 1.0 - torch.rand((what, n_r, n_e), dtype=torch.float64, device="cuda", generator=gen)
                    total = torch.ones((n_r, n_e), dtype=torch.float64, device="cuda")
                    torch.cuda.synchronize()
                    rt.set_source_channels_device(rates.data_ptr(), total.data_ptr(), what, n_r, n_e)
                    del rates, total
                for mode in ("f64", "fixed64"):
                    rt.set_accumulation_mode(mode)
                    p = rt.shells_params(n, seed=1, spectra=True)
                    n_acc = 256 * 256 + L.SART_ACC_COUNT + 2 * p.n_radial_bins + 3 * (n_e + 1)
                    acc = torch.zeros(n_acc, dtype=torch.float64, device="cuda")
                    if what == "shells":
                        blk = torch.zeros(rt.shell_block_len(True), dtype=torch.float64, device="cuda")
                        ms = timed(lambda: rt.trace_shells_device(p, acc.data_ptr(), blk.data_ptr()))
                    elif what == "origin":
                        blk = torch.zeros(rt.origin_block_len(), dtype=torch.float64, device="cuda")
                        ms = timed(lambda: rt.trace_origin_device(p, acc.data_ptr(), blk.data_ptr()))
                    elif isinstance(what, int):
                        blk = torch.zeros(rt.channel_block_len(True, 256), dtype=torch.float64, device="cuda")
                        ms = timed(lambda: rt.trace_channels_device(p, acc.data_ptr(), blk.data_ptr()))
                    else:
                        ms = timed(lambda: rt.trace_histogram_device(p, acc.data_ptr()))
                    results[(label, mode)] = ms * 1e9 / n
            finally:
                rt.close()
    print("babyiaxo_xmm, %d x %d tables, %d rays per launch, median of %d; ms per 1e9 rays (ratio to hist generic); library %s"
          % (n_r, n_e, n, repeats, os.path.basename(L.LIBSART_PATH)))
    for mode in ("f64", "fixed64"):
        base = results[("hist generic", mode)]
        print("%-8s " % mode + "  ".join("%s %8.2f (%.2f x)" % (label, results[(label, mode)], results[(label, mode)] / base)
                                         for label, _, _ in labels), flush=True)


main()
