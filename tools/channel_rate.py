#!/usr/bin/env python3
"""Kernel time per 1e9 rays of the emission-channel breakdown (sart_trace_histogram_channels_device) at T = 3 and T = 8 channels
against the per-shell entry and the plain histogram entry on the same box, the same rays and full-size tables (1968 x 1500: the
fraction table is 1968 x 1500 x stride doubles, 94 MB at stride 4 and 189 MB at stride 8):
    python tools/channel_rate.py [rays] [repeats]

BabyIAXO / XMM, f64 and FIXED64, image 256 x 256 with spectra (10 000 radial bins).  Per case, the median of `repeats` warm runs
between two HIP events (launch + folds):
  hist            the histogram entry as shipped (the specialised kernel variant of the setup)
  hist generic    the same with SART_FORCE_GENERIC (the generic variant, which the shell and channel kernels are built on; this
                  change leaves that kernel as it was)
  shells          the per-shell entry
  channels T=3    the channel entry, three channels (stride 4)
  channels T=8    the channel entry, eight channels (stride 8)
The fractions are uniform random numbers in (0, 1]: every channel of every passed ray issues its atomics."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import solaraxionraytracing_amd as sa
from solaraxionraytracing_amd import _lib as L

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
    labels = (("hist", {}, None), ("hist generic", {"SART_FORCE_GENERIC": "1"}, None), ("shells", {}, "shells"),
              ("channels T=3", {}, 3), ("channels T=8", {}, 8))
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
                    elif isinstance(what, int):
                        blk = torch.zeros(rt.channel_block_len(True, 256), dtype=torch.float64, device="cuda")
                        ms = timed(lambda: rt.trace_channels_device(p, acc.data_ptr(), blk.data_ptr()))
                    else:
                        ms = timed(lambda: rt.trace_histogram_device(p, acc.data_ptr()))
                    results[(label, mode)] = ms * 1e9 / n
            finally:
                rt.close()
    print("babyiaxo_xmm, %d x %d tables, %d rays per launch, median of %d; ms per 1e9 rays (ratio to hist generic)" % (n_r, n_e, n, repeats))
    for mode in ("f64", "fixed64"):
        base = results[("hist generic", mode)]
        print("%-8s " % mode + "  ".join("%s %8.2f (%.2f x)" % (label, results[(label, mode)], results[(label, mode)] / base)
                                         for label, _, _ in labels), flush=True)


main()
