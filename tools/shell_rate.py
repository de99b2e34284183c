#!/usr/bin/env python3
"""Time per 1e9 rays of the per-shell breakdown (sart_trace_histogram_shells_device) against the plain histogram entry
(sart_trace_histogram_device) on the same params:  python tools/shell_rate.py [rays] [repeats]

Setups: BabyIAXO / XMM and CAST / LLNL with its four coatings (tests/conftest.py's make_setup / SMALL tables); f64 and FIXED64; with
and without spectra (10 000 radial bins).  Per case, the median of `repeats` warm runs between two HIP events (launch + folds):
  hist            the histogram entry as shipped (the specialised kernel variant of the setup)
  hist generic    the same with SART_FORCE_GENERIC (the generic variant, which the shell kernel is built on)
  shells          the shell entry (LDS image tile narrowed to 53 x 53 / 28 x 28 for the shell table)
  shells no tile  the shell entry with SART_NO_IMAGE_TILE (every pixel a global atomic, no pilot launch: the other LDS option)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import solaraxionraytracing_amd as sa
from solaraxionraytracing_amd import _lib as L
from tests.conftest import SMALL, make_setup

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


def case(name, full):
    results = {}
    for label, env, shells in (("hist", {}, False), ("hist generic", {"SART_FORCE_GENERIC": "1"}, False), ("shells", {}, True),
                               ("shells no tile", {"SART_NO_IMAGE_TILE": "1"}, True)):
        with torch.cuda.stream(stream):
            rt = tracer(full, env)
            try:
                rt.set_stream(stream.cuda_stream)
                for mode in ("f64", "fixed64"):
                    rt.set_accumulation_mode(mode)
                    for spectra in (False, True):
                        p = rt.shells_params(n, seed=1, spectra=spectra)
                        n_acc = 256 * 256 + L.SART_ACC_COUNT + ((2 * p.n_radial_bins + 3 * (full.energies.size + 1)) if spectra else 0)
                        acc = torch.zeros(n_acc, dtype=torch.float64, device="cuda")
                        blk = torch.zeros(rt.shell_block_len(spectra), dtype=torch.float64, device="cuda")
                        if shells:
                            ms = timed(lambda: rt.trace_shells_device(p, acc.data_ptr(), blk.data_ptr()))
                        else:
                            ms = timed(lambda: rt.trace_histogram_device(p, acc.data_ptr()))
                        results[(label, mode, spectra)] = ms * 1e9 / n
            finally:
                rt.close()
    for mode in ("f64", "fixed64"):
        for spectra in (False, True):
            base = results[("hist", mode, spectra)]
            print("%-14s %-7s spectra %-5s " % (name, mode, spectra) + "  ".join(
                "%s %8.2f ms (%.2f x)" % (label, results[(label, mode, spectra)], results[(label, mode, spectra)] / base)
                for label in ("hist", "hist generic", "shells", "shells no tile")) + "   [ms per 1e9 rays]", flush=True)


case("babyiaxo_xmm", make_setup("babyiaxo_xmm"))
case("cast_llnl", sa.initFullSetup(L.ES_CAST, L.DK_INGRID2018, L.SK_VACUUM, L.TK_LLNL, **SMALL))
