#!/usr/bin/env python3
"""(ray, angle)/s of the fused angular scan with per-angle images against the flux-only scan and a host loop of single image launches
(BabyIAXO / XMM, default tables and flags, angles 0.01 .. 0.3 deg):  python tools/ascan_images_rate.py [rays] [repeats]

Two chips: the default 14 mm (beyond ~0.1 deg the spot leaves the chip: few pixel atomics) and 100 mm (ChipXMax = 100 mm,
raytracer.nim:262-264: the spot stays on the 256 x 256 image at every angle - every passed (ray, angle) pays its pixel atomic).

  (a) flux-only fused scan           sart_trace_angular_scan_device
  (b) fused scan with images         sart_trace_angular_scan_images_device, 256 x 256
  (c) ... with images and spectra    the same with params.spectra (10 000 radial bins)
  (d) host loop of image launches    per angle sart_set_telescope_angles + sart_trace_histogram_device (its pilot launch included)

Every configuration is run once to warm up, then `repeats` times between two HIP events on the context's stream (a torch stream:
sart_set_stream); the median is printed.  FIXED64 and f64 accumulation are timed both (f64 is the default mode)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import solaraxionraytracing_amd as sa
from solaraxionraytracing_amd.raytracer import angular_scan_len

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_000_000_000
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
        if r:   # the first run warms up
            ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def run(chip):
    full = sa.initFullSetup()
    full.setup.chip_x_max = full.setup.chip_y_max = chip
    with torch.cuda.stream(stream), sa.RayTracer(full) as rt:
        rt.set_stream(stream.cuda_stream)
        for mode in ("f64", "fixed64"):
            rt.set_accumulation_mode(mode)
            for k in (16, 32):
                an = np.linspace(0.01, 0.3, k)
                rows = torch.zeros(angular_scan_len(k), dtype=torch.float64, device="cuda")
                p = rt.trace_params(n, seed=1)
                ps = rt.angular_scan_images_params(n, seed=1, spectra=True)
                blocks = torch.zeros(k * (256 * 256 + 24), dtype=torch.float64, device="cuda")
                blocks_s = torch.zeros(k * (256 * 256 + 24 + 2 * 10_000 + 3 * (full.energies.size + 1)), dtype=torch.float64, device="cuda")
                acc = torch.zeros(256 * 256 + 24, dtype=torch.float64, device="cuda")
                y0 = full.setup.telescope_turned_y_deg

                def host_loop():
                    for a in an:
                        rt.set_telescope_angles(turned_y_deg=float(a))
                        rt.trace_histogram_device(p, acc.data_ptr())
                    rt.set_telescope_angles(turned_y_deg=y0)

                res = {
                    "a_flux_only_scan": timed(lambda: rt.trace_angular_scan_device(p, an, rows.data_ptr())),
                    "b_images_scan": timed(lambda: rt.trace_angular_scan_images_device(p, an, rows.data_ptr(), blocks.data_ptr())),
                    "c_images_spectra_scan": timed(lambda: rt.trace_angular_scan_images_device(ps, an, rows.data_ptr(), blocks_s.data_ptr())),
                    "d_host_loop_image_launches": timed(host_loop),
                }
                for name, ms in res.items():
                    print("chip %3.0f mm  %-8s %2d angles  %-28s %9.3f ms  %.3e (ray, angle)/s" % (chip, mode, k, name, ms, n * k / (ms / 1e3)), flush=True)
                print("chip %3.0f mm  %-8s %2d angles  (b) / (d) speed-up %.2f x, (b) / (a) %.2f" % (
                    chip, mode, k, res["d_host_loop_image_launches"] / res["b_images_scan"], res["a_flux_only_scan"] / res["b_images_scan"]), flush=True)


for chip in (14.0, 100.0):
    run(chip)
