#!/usr/bin/env python3
"""(ray, energy) evaluations per second of the fused energy scan (sart_trace_energy_scan) at K = 8, 32 and 99 energies, against the
host loop it replaces (per energy: sart_set_setup with that test_energy, then a sart_trace_histogram_device launch - what
tests/test_reference_data.py's DTU-curve test does):  python tools/energy_scan_rate.py [rays] [repeats]

Two setups:  CAST / LLNL, gold, parallel beam of the bore's 21.5 mm (the DTU effective-area configuration: window, gas and
conversion factors off) on the default tables, and the `babyiaxo_xmm_xray` setup of tests/conftest.py (BabyIAXO / XMM, the
default X-ray test source, small tables).

  scan                 sart_trace_energy_scan_device, f64 and FIXED64, median of `repeats` runs between two HIP events (warm)
  host loop, kernels   the single launches' own kernel time (sart_enable_kernel_timing), K = 32
  host loop, wall      the same loop on the wall clock: the table rebuild of every sart_set_setup (hoist_energy_tables +
                       hoist_reflectivity, uploads) included, K = 32"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import solaraxionraytracing_amd as sa
from solaraxionraytracing_amd import _lib as L
from tests.conftest import make_setup

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 3
stream = torch.cuda.Stream()
DTU_FLAGS = L.CF_XRAY_TEST | L.CF_IGNORE_DET_WINDOW | L.CF_IGNORE_GAS_ABS | L.CF_IGNORE_CONV_PROB


def timed(fn):
    ms = []
    for r in range(repeats + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        if r:   # the first run warms up
            ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def cast_llnl_gold_parallel():
    src = L.TestSourceConfig()
    src.active, src.parallel = 1, 1
    src.energy, src.distance, src.radius, src.activity = 1.0, 100.0, 21.5, 1.0
    src.offAxisUp = src.offAxisLeft = src.lengthCol = 0.0
    return sa.initFullSetup(L.ES_CAST, L.DK_INGRID2018, L.SK_VACUUM, L.TK_LLNL, flags=DTU_FLAGS, source_cfg=src, reflectivity="gold")


def run(name, full, flags):
    with torch.cuda.stream(stream), sa.RayTracer(full) as rt:
        rt.set_stream(stream.cuda_stream)
        p = rt.trace_params(n, seed=1, flags=flags)
        scan_ms = {}
        for mode in ("f64", "fixed64"):
            rt.set_accumulation_mode(mode)
            for k in (8, 32, 99):
                es = np.linspace(0.5, 10.0, k)
                rows = torch.zeros(L.energy_scan_len(k), dtype=torch.float64, device="cuda")
                ms = timed(lambda: rt.trace_energy_scan_device(p, es, rows.data_ptr()))
                scan_ms[(mode, k)] = ms
                print("%-18s %-8s K = %2d  scan %10.3f ms  %.3e (ray, energy)/s" % (name, mode, k, ms, n * k / (ms / 1e3)), flush=True)
        # the host loop of single launches, K = 32, f64
        rt.set_accumulation_mode("f64")
        es = np.linspace(0.5, 10.0, 32)
        acc = torch.zeros(sa.accumulator_len(256), dtype=torch.float64, device="cuda")
        s0 = L.Setup()
        L.check(rt.lib.sart_get_setup(rt.handle, C.byref(s0)))

        def host_loop():
            for e in es:
                s = L.Setup.from_buffer_copy(s0)
                s.test_energy = float(e)
                L.check(rt.lib.sart_set_setup(rt.handle, C.byref(s)))
                rt.trace_histogram_device(p, acc.data_ptr())
            L.check(rt.lib.sart_set_setup(rt.handle, C.byref(s0)))

        host_loop()   # warm-up
        torch.cuda.synchronize()
        rt.enable_kernel_timing(True)
        t0 = time.perf_counter()
        host_loop()
        stream.synchronize()
        wall_ms = (time.perf_counter() - t0) * 1e3
        kern_ms, n_launch = rt.kernel_timing()
        rt.enable_kernel_timing(False)
        s_ms = scan_ms[("f64", 32)]
        print("%-18s host loop K = 32: kernels %10.3f ms (%d launches, %.3e (ray, energy)/s), wall %10.3f ms (%.3e /s)" % (
            name, kern_ms, n_launch, n * 32 / (kern_ms / 1e3), wall_ms, n * 32 / (wall_ms / 1e3)), flush=True)
        print("%-18s K = 32 speed-up of the f64 scan: %.2f x over the host loop's kernel time, %.2f x over its wall time" % (
            name, kern_ms / s_ms, wall_ms / s_ms), flush=True)


run("cast_llnl_gold_par", cast_llnl_gold_parallel(), DTU_FLAGS)
run("babyiaxo_xmm_xray", make_setup("babyiaxo_xmm_xray"), L.CF_XRAY_TEST)
