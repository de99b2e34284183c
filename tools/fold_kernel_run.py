#!/usr/bin/env python3
"""Runs every fold and finalize kernel a few times, for a kernel trace of a build (the folds run for microseconds behind
millisecond traces; bench.py's trace shows only the scalars fold):

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/fold_kernel_run.py
  python3 tools/fold_kernel_run.py --table PARENT_kernel_stats.csv NEW_kernel_stats.csv      (no GPU: parent beside new)

The run: the blocking form of every fused entry on the small tables, 2e5 rays, in f64 and in FIXED64 (whose blocking forms
finalize), REPEATS times each.  SART_LIBSART selects another build's library."""
import csv
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, REPEATS = 200_000, 5


def run():
    import numpy as np
    from tests.conftest import SMALL, make_setup
    import solaraxionraytracing_amd as sa
    from solaraxionraytracing_amd import tables
    for mode in ("f64", "fixed64"):
        with sa.RayTracer(make_setup("babyiaxo_xmm")) as rt:
            rt.set_accumulation_mode(mode)
            total = tables.primakoff_emission_table(SMALL["n_radii"], SMALL["n_energies"])
            rt.set_source_channels(np.random.default_rng(1).random((3,) + total.shape) * total, total)
            rt.set_aperture_grid(48, 20, -352.0, 352.0, -352.0, 352.0)
            for _ in range(REPEATS):
                rt.trace_spectra(N, seed=7, n_radial_bins=100)
                rt.trace_shells(N, seed=7, n_radial_bins=100)
                rt.trace_channels(N, seed=7, n_radial_bins=100)
                rt.trace_origin(N, seed=7, n_radial_bins=100)
                rt.trace_aperture(N, seed=7, n_radial_bins=100)
                rt.trace_angular_scan(np.linspace(0.0, 0.3, 5), N, seed=7)
                rt.trace_angular_scan_images(np.linspace(0.0, 0.3, 3), N, seed=7, image_n=64)
        with sa.RayTracer(make_setup("babyiaxo_xmm_gas")) as rt:
            rt.set_accumulation_mode(mode)
            for _ in range(REPEATS):
                rt.trace_mass_scan(np.linspace(0.002, 0.03, 33), N, seed=7)
                rt.trace_mass_scan_spectra(np.linspace(0.002, 0.03, 33), (20, 6, 15), N, seed=7)
        with sa.RayTracer(make_setup("babyiaxo_xmm_xray")) as rt:
            rt.set_accumulation_mode(mode)
            for _ in range(REPEATS):
                rt.trace_energy_scan(np.array([0.5, 1.5, 3.0, 6.0, 9.0]), N, seed=7)


def table(parent_csv, new_csv):
    def read(path):
        return {r["Name"]: r for r in csv.DictReader(open(path)) if "fold_" in r["Name"] or "finalize_" in r["Name"] or "fixed_check" in r["Name"]}
    a, b = read(parent_csv), read(new_csv)
    print("%-118s %6s %22s %22s" % ("kernel (rocprofv3 --kernel-trace --stats; ns)", "calls", "parent avg / min", "new avg / min"))
    for name in sorted(set(a) | set(b)):
        cell = lambda r: "%10.0f / %9.0f" % (float(r["AverageNs"]), float(r["MinNs"])) if r else "%22s" % "-"
        calls = (b.get(name) or a.get(name))["Calls"]
        print("%-118s %6s %22s %22s" % (name[:118], calls, cell(a.get(name)), cell(b.get(name))))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--table":
        table(sys.argv[2], sys.argv[3])
    else:
        run()
