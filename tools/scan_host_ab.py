#!/usr/bin/env python3
"""Host cost of the fused scans' entry points, two builds side by side:  python tools/scan_host_ab.py OLD/libsart.so NEW/libsart.so [rounds]

Each library runs in a child process of its own, the two alternating `rounds` times (default 3).  A child times, on the gas-stage
setup with the X-ray test source (small tables: the one setup the mass, the energy and the angular scan all accept),

  back to back   the wall time of 200 accumulating `_device` calls of 1e5 rays each with ONE synchronise at the end - mass scan
                 (32 masses), energy scan (32 energies), angular scan (16 angles): what a stream synchronisation or an allocation
                 that a call did not have before would add to;
  kernel bound   the wall time, synchronise included, of one call of 1e8 rays - energy scan at 32 energies, angular scan with
                 256 x 256 images at 16 angles - median of 3.

Prints every child's JSON line, then per figure the median of each library, the spread (max - min) of each and the difference."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child():
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import solaraxionraytracing_amd as sa
    from solaraxionraytracing_amd import _lib as L
    from solaraxionraytracing_amd.raytracer import angular_scan_len, mass_scan_len
    from tests.conftest import SMALL

    full = sa.initFullSetup(stage=L.SK_GAS, flags=L.CF_XRAY_TEST, **SMALL)
    masses = np.linspace(0.0, 0.05, 32)
    energies = np.linspace(0.3, 12.0, 32)
    angles = np.linspace(0.0, 0.05, 16)
    out = {"lib": os.environ.get("SART_LIBSART", "")}
    with sa.RayTracer(full) as rt:
        def wall(call, n_calls, n_rays):
            call(rt.trace_params(n_rays, seed=1, ray_id_offset=0, accumulate=False))   # warm: scratch, occupancy query, tables
            rt.synchronize()
            t0 = time.perf_counter()
            for k in range(n_calls):
                call(rt.trace_params(n_rays, seed=1, ray_id_offset=(k + 1) * n_rays, accumulate=True))
            rt.synchronize()
            return (time.perf_counter() - t0) * 1e3

        m_acc = torch.zeros(mass_scan_len(32), dtype=torch.float64, device="cuda")
        e_acc = torch.zeros(L.energy_scan_len(32), dtype=torch.float64, device="cuda")
        a_acc = torch.zeros(angular_scan_len(16), dtype=torch.float64, device="cuda")
        mass = lambda p: rt.trace_mass_scan_device(p, masses, m_acc.data_ptr())
        energy = lambda p: rt.trace_energy_scan_device(p, energies, e_acc.data_ptr())
        angular = lambda p: rt.trace_angular_scan_device(p, angles, a_acc.data_ptr())
        for name, call in (("mass32_200x1e5_ms", mass), ("energy32_200x1e5_ms", energy), ("angular16_200x1e5_ms", angular)):
            out[name] = wall(call, 200, 100_000)
        out["energy32_1e8_ms"] = statistics.median(wall(energy, 1, 100_000_000) for _ in range(3))
        blen = sa.accumulator_len(256)
        blocks = torch.zeros(16 * blen, dtype=torch.float64, device="cuda")

        def images(p):
            q = rt.angular_scan_images_params(p.n_rays, p.seed, p.ray_id_offset, None, 256, False, 0, 10.0, bool(p.accumulate))
            rt.trace_angular_scan_images_device(q, angles, a_acc.data_ptr(), blocks.data_ptr())
        out["images16_1e8_ms"] = statistics.median(wall(images, 1, 100_000_000) for _ in range(3))
    print(json.dumps(out), flush=True)


def main():
    libs = [os.path.abspath(p) for p in sys.argv[1:3]]
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    runs = {lib: [] for lib in libs}
    for _ in range(rounds):
        for lib in libs:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=dict(os.environ, SART_LIBSART=lib),
                               capture_output=True, text=True, timeout=280)
            if r.returncode != 0:
                sys.exit("child failed (%d) with %s:\n%s" % (r.returncode, lib, r.stderr[-2000:]))
            line = r.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            runs[lib].append(json.loads(line))
    old, new = libs
    for key in [k for k in runs[old][0] if k != "lib"]:
        a, b = [r[key] for r in runs[old]], [r[key] for r in runs[new]]
        print("%-22s old %9.3f (spread %7.3f)  new %9.3f (spread %7.3f)  new - old %+8.3f" %
              (key, statistics.median(a), max(a) - min(a), statistics.median(b), max(b) - min(b), statistics.median(b) - statistics.median(a)))


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
