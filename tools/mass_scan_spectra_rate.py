#!/usr/bin/env python3
"""Time of the banded mass scan (sart_trace_mass_scan_spectra) beside what it stands between: the plain fused scan it extends and the
host loop of single-mass spectra launches it replaces.  python tools/mass_scan_spectra_rate.py [rays] [repeats] [--parent LIBSART]

BabyIAXO / XMM in the gas stage on the default (full-size) tables, 32 masses (one launch group), f64 and FIXED64, one process:

  (a) plain      sart_trace_mass_scan_device
  (b) bands N    sart_trace_mass_scan_spectra_device at N = 1, 8 and 31 bands over the whole energy table (N = 1: every passed lane
                 of a wave adds to ONE LDS cell per mass and quantity, the worst case of same-address serialisation)
  (c) host loop  32 x (sart_set_axion_mass, sart_trace_histogram_device with spectra, accumulate = 0): what gives the spectrum per
                 mass without the banded scan

Each figure: median and spread (max - min) of `repeats` warm timings between two HIP events on the context's stream, in ms per scan;
a timing of (a) or (b) spans --inner scans back to back (one scan of 1e9 rays takes some 20 ms).
--parent LIBSART: --parent-measure (default (a) and (c)) also with that libsart.so (a build of the parent commit), in child
processes of this one that take turns with it - parent, this build, parent, this build - so that both see the same box in the same
minutes."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("rays", nargs="?", type=float, default=3e8)
ap.add_argument("repeats", nargs="?", type=int, default=5)
ap.add_argument("--parent", default="", help="libsart.so of the parent commit")
ap.add_argument("--inner", type=int, default=5, help="scans per timing of (a) and (b)")
ap.add_argument("--parent-measure", default="plain,loop", help="what the --parent comparison times: plain, loop or both")
ap.add_argument("--measure", default="plain,bands,loop", help="(child runs) what to time")
ap.add_argument("--json", action="store_true", help="(child runs) print one JSON line instead of the table")
args = ap.parse_args()
n, repeats, what = int(args.rays), args.repeats, args.measure.split(",")

import torch  # noqa: E402  (before the library: torch brings the HIP runtime both use)

import solaraxionraytracing_amd as sa  # noqa: E402
from solaraxionraytracing_amd import _lib as L  # noqa: E402

if "SART_LIBSART" in os.environ:   # a library of another commit: bind what it has
    have = C.CDLL(L.LIBSART_PATH)
    L.SART_SYMBOLS = {k: v for k, v in L.SART_SYMBOLS.items() if hasattr(have, k)}

MASSES = np.linspace(0.0, 0.02, 32)
BANDS = (1, 8, 31)
NR = 10_000


def timed(stream, fn, inner=1):
    ms = []
    for r in range(repeats + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(inner):
            fn()
        b.record(stream)
        b.synchronize()
        if r:   # the first run warms up
            ms.append(a.elapsed_time(b) / inner)
    return float(np.median(ms)), float(max(ms) - min(ms))


def measure():
    full = sa.initFullSetup(stage=L.SK_GAS)
    n_e = full.energies.size
    out = {}
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream), sa.RayTracer(full) as rt:
        rt.set_stream(stream.cuda_stream)
        for mode in ("f64", "fixed64"):
            rt.set_accumulation_mode(mode)
            p = rt.trace_params(n, seed=1)
            rows = torch.zeros(sa.mass_scan_len(32), dtype=torch.float64, device="cuda")
            if "plain" in what:
                out[mode + " plain"] = timed(stream, lambda: rt.trace_mass_scan_device(p, MASSES, rows.data_ptr()), args.inner)
            if "bands" in what:
                for nb in BANDS:
                    bands = (0, n_e // nb, nb)
                    spec = torch.zeros(L.mass_scan_spectra_len(32, nb), dtype=torch.float64, device="cuda")
                    out[mode + " bands %d" % nb] = timed(stream, lambda: rt.trace_mass_scan_spectra_device(p, MASSES, bands, rows.data_ptr(), spec.data_ptr()), args.inner)
            if "loop" in what:
                ps = rt.trace_params(n, seed=1)
                ps.spectra, ps.n_radial_bins, ps.radial_max = 1, NR, 10.0
                acc = torch.zeros(256 * 256 + L.SART_ACC_COUNT + 2 * NR + 3 * (n_e + 1), dtype=torch.float64, device="cuda")

                def host_loop():
                    for m in MASSES:
                        rt.set_axion_mass(float(m))
                        rt.trace_histogram_device(ps, acc.data_ptr())

                out[mode + " loop"] = timed(stream, host_loop)
                rt.set_axion_mass(float(full.setup.m_axion))
        rt.synchronize()
    return out


def child(lib):
    env = dict(os.environ)
    if lib:
        env["SART_LIBSART"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(n), str(repeats), "--inner", str(args.inner), "--measure",
                        args.parent_measure, "--json"],
                       env=env, capture_output=True, text=True, timeout=1500)
    if r.returncode != 0:
        raise SystemExit("child run failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def show(title, res):
    for mode in ("f64", "fixed64"):
        keys = [k for k in res if k.startswith(mode + " ")]
        print("%-22s %-8s " % (title, mode) + "  ".join("%s %9.2f +- %5.2f" % (k[len(mode) + 1:], *res[k]) for k in keys), flush=True)


if args.json:
    print(json.dumps(measure()))
    sys.exit(0)

print("babyiaxo_xmm gas stage, default tables, 32 masses, %d rays per scan, %d repeats of %d scans (host loop: of 1); ms per scan: "
      "median +- spread" % (n, repeats, args.inner), flush=True)
if args.parent:
    show("parent, run 1", child(args.parent))
    show("this build (child), 1", child(""))
    show("parent, run 2", child(args.parent))
    show("this build (child), 2", child(""))
res = measure()
show("this build", res)
for mode in ("f64", "fixed64"):
    a, c = res[mode + " plain"][0], res[mode + " loop"][0]
    for nb in BANDS:
        b = res[mode + " bands %d" % nb][0]
        print("%-8s bands %2d: %.3f x the plain scan (a), %.2f x faster than the host loop (c)%s" % (
            mode, nb, b / a, c / b, "" if b < c else "   SLOWER THAN THE HOST LOOP"), flush=True)
