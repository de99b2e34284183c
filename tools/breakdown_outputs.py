#!/usr/bin/env python3
"""Outputs of the breakdown and scan entries of one build, for a parent / new comparison of two builds on the same box:

  SART_LIBSART=<parent .so> python tools/breakdown_outputs.py dump parent.npz
  python tools/breakdown_outputs.py dump new.npz
  python tools/breakdown_outputs.py compare parent.npz new.npz [--json OUT] [--parent-again parent2.npz]

dump: the five setups of tests/test_gpu_shells.py at that test's shape (400 000 rays, seed 7, offset 13, image 256 x 256 with
spectra).  FIXED64: the raw int64 accumulator and block of a shells launch, of a channels launch at T = 3 and T = 8 (random
fractions), of an origin launch (neither for the X-ray test source, which has no solar draw) and of an aperture launch (48 x 20
cells); and one small scan of each kind - 33 masses plain and with 15 energy bands (gas stage), 5 energies (X-ray source), 5 angles
and 3 angles with 64 x 64 images - as the raw rows, cells and blocks.  f64: the scalars and the rows / heads of the same launches;
of the scans the counters and the sums.
compare: every FIXED64 array byte for byte; in f64 every counter equal and the largest relative difference of the sums - with
--parent-again (a second dump of the parent in the same session: the f64 partials follow the order of LDS atomics and differ from
run to run) that difference may not exceed the largest one between the two parent dumps.  Exit status 1 unless all of that holds."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from solaraxionraytracing_amd import _lib as L   # noqa: E402

N, SEED, OFF, IMAGE_N = 400_000, 7, 13, 256


def dump(path):
    import torch
    from tests import test_gpu_channels as TC
    from tests import test_gpu_shells as TS
    out = {}
    for name in TS.CASES:
        with TS.Tracer(TS.setup_of(name)) as rt:
            for mode, dtype in (("fixed64", torch.int64), ("f64", torch.float64)):
                rt.set_accumulation_mode(mode)
                launches = [("shells", 0)] + ([] if rt.full.setup.test_active else [("channels", 3), ("channels", 8)])
                for kind, t in launches:
                    if t:
                        rt.set_source_channels(TC.random_fractions(t), np.ones(TC.total_table().shape))
                    p = TC.params(rt, N, SEED, OFF, True, IMAGE_N, accumulate=True)
                    acc = TC.zeros(torch, TC.acc_len(rt, p), dtype)
                    blk = TC.zeros(torch, rt.channel_block_len(True, IMAGE_N) if t else rt.shell_block_len(True), dtype)
                    (rt.trace_channels_device if t else rt.trace_shells_device)(p, acc.data_ptr(), blk.data_ptr())
                    rt.synchronize()
                    key = "%s/%s/%s%s" % (name, mode, kind, t or "")
                    acc, blk = acc.cpu().numpy(), blk.cpu().numpy()
                    if mode == "fixed64":
                        out[key + "/acc"], out[key + "/block"] = acc, blk
                    else:   # the image and the spectra follow the order of the f64 atomics: the scalars and the rows
                        rows = t or rt.full.setup.n_shells
                        out[key + "/scalars"] = acc[IMAGE_N * IMAGE_N:IMAGE_N * IMAGE_N + L.SART_ACC_COUNT]
                        out[key + "/rows"] = blk[:rows * L.SHELL_ROW].reshape(rows, L.SHELL_ROW)
                if not rt.full.setup.test_active:
                    head_block(rt, torch, out, "%s/%s/origin" % (name, mode), dtype, rt.origin_block_len(), rt.trace_origin_device)
                rt.set_aperture_grid(48, 20, -352.0, 352.0, -352.0, 352.0)
                head_block(rt, torch, out, "%s/%s/aperture" % (name, mode), dtype, rt.aperture_block_len(), rt.trace_aperture_device)
    scans(torch, out)
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays; build", L.build_id())


def head_block(rt, torch, out, key, dtype, n_slots, trace):
    """One origin or aperture launch: raw arrays in FIXED64; in f64 the scalars and the head (the cells take atomics, no fold)."""
    from tests import test_gpu_channels as TC
    p = TC.params(rt, N, SEED, OFF, True, IMAGE_N, accumulate=True)
    acc, blk = TC.zeros(torch, TC.acc_len(rt, p), dtype), TC.zeros(torch, n_slots, dtype)
    trace(p, acc.data_ptr(), blk.data_ptr())
    rt.synchronize()
    acc, blk = acc.cpu().numpy(), blk.cpu().numpy()
    if dtype == torch.int64:
        out[key + "/acc"], out[key + "/block"] = acc, blk
    else:
        out[key + "/scalars"] = acc[IMAGE_N * IMAGE_N:IMAGE_N * IMAGE_N + L.SART_ACC_COUNT]
        out[key + "/counters"], out[key + "/sums"] = blk[:1], blk[1:3]


def scans(torch, out):
    """One small scan of each kind (rows of 8 slots: the two sums, then counters; the counter row behind them)."""
    from tests import test_gpu_channels as TC
    from tests import test_gpu_shells as TS
    n_scan, image_n = 200_000, 64

    def rows_of(key, buf, n, dtype):
        r = buf.cpu().numpy()
        if dtype == torch.int64:
            out[key + "/rows"] = r
        else:
            r = r.reshape(n + 1, 8)
            out[key + "/sums"], out[key + "/counters"] = r[:n, :2].copy(), np.concatenate([r[:n, 2:].reshape(-1), r[n]])

    masses, bands = np.linspace(0.002, 0.03, 33), (20, 6, 15)
    energies, angles = np.array([0.5, 1.5, 3.0, 6.0, 9.0]), np.array([0.0, 0.05, -0.1, 0.2, 0.5])
    for mode, dtype in (("fixed64", torch.int64), ("f64", torch.float64)):
        with TS.Tracer(TS.setup_of("babyiaxo_xmm_gas"), generic=False) as rt:
            rt.set_accumulation_mode(mode)
            p = rt.trace_params(n_scan, SEED, OFF, accumulate=True)
            rows = TC.zeros(torch, 34 * 8, dtype)
            rt.trace_mass_scan_device(p, masses, rows.data_ptr())
            rt.synchronize()
            rows_of("scan/%s/mass" % mode, rows, 33, dtype)
            rows, spec = TC.zeros(torch, 34 * 8, dtype), TC.zeros(torch, L.mass_scan_spectra_len(33, bands[2]), dtype)
            rt.trace_mass_scan_spectra_device(p, masses, bands, rows.data_ptr(), spec.data_ptr())
            rt.synchronize()
            rows_of("scan/%s/banded" % mode, rows, 33, dtype)
            spec = spec.cpu().numpy()
            if dtype == torch.int64:
                out["scan/%s/banded/cells" % mode] = spec
            else:
                spec = spec.reshape(34, bands[2] + 1, L.MSPEC_CELL)
                out["scan/%s/banded_cells/sums" % mode], out["scan/%s/banded_cells/counters" % mode] = spec[:33, :, :2].copy(), spec[33, :, 0].copy()
        with TS.Tracer(TS.setup_of("babyiaxo_xmm_xray"), generic=False) as rt:
            rt.set_accumulation_mode(mode)
            rows = TC.zeros(torch, 6 * 8, dtype)
            rt.trace_energy_scan_device(rt.trace_params(n_scan, SEED, OFF, accumulate=True), energies, rows.data_ptr())
            rt.synchronize()
            rows_of("scan/%s/energy" % mode, rows, 5, dtype)
        with TS.Tracer(TS.setup_of("babyiaxo_xmm"), generic=False) as rt:
            rt.set_accumulation_mode(mode)
            rows = TC.zeros(torch, 6 * 8, dtype)
            rt.trace_angular_scan_device(rt.trace_params(n_scan, SEED, OFF, accumulate=True), angles, rows.data_ptr())
            rt.synchronize()
            rows_of("scan/%s/angular" % mode, rows, 5, dtype)
            blen = image_n * image_n + L.SART_ACC_COUNT
            rows, blocks = TC.zeros(torch, 4 * 8, dtype), TC.zeros(torch, 3 * blen, dtype)
            rt.trace_angular_scan_images_device(rt.angular_scan_images_params(n_scan, SEED, OFF, image_n=image_n, accumulate=True), angles[:3],
                                                rows.data_ptr(), blocks.data_ptr())
            rt.synchronize()
            rows_of("scan/%s/angular_images" % mode, rows, 3, dtype)
            blocks = blocks.cpu().numpy().reshape(3, blen)
            if dtype == torch.int64:
                out["scan/%s/angular_images/blocks" % mode] = blocks
            else:
                out["scan/%s/angular_images/scalars" % mode] = blocks[:, image_n * image_n:].copy()


def f64_differences(a, b):
    """(every counter equal, largest relative difference of the sums, where, how many sums differ at all) between two dumps."""
    counters_equal, worst, worst_key, n_differ = True, 0.0, None, 0
    for k in (k for k in a.files if "/f64/" in k):
        kind = k.split("/")[2]
        x, y = a[k].reshape(-1, a[k].shape[-1]), b[k].reshape(-1, b[k].shape[-1])
        if k.endswith("/counters"):
            counters_equal &= bool(np.array_equal(x, y))
            continue
        names = {"all": slice(None)} if k.endswith("/sums") else L.ACC if k.endswith("/scalars") else L.SHELL if kind == "shells" else L.CHAN
        for key, slot in names.items():
            if key.startswith("N_"):
                counters_equal &= bool(np.array_equal(x[:, slot], y[:, slot]))
            else:
                d = np.abs(x[:, slot] - y[:, slot])
                n_differ += int(np.count_nonzero(d))
                rel = float(np.max(np.where(x[:, slot] != 0, d / np.where(x[:, slot] != 0, np.abs(x[:, slot]), 1.0), d)))
                if rel > worst:
                    worst, worst_key = rel, "%s %s" % (k, key)
    return counters_equal, worst, worst_key, n_differ


def compare(a_path, b_path, json_path, again_path=None):
    a, b = np.load(a_path), np.load(b_path)
    assert sorted(a.files) == sorted(b.files)
    fixed = {k: bool(a[k].tobytes() == b[k].tobytes()) for k in a.files if "/fixed64/" in k}
    counters_equal, worst, worst_key, n_differ = f64_differences(a, b)
    out = {"shape": {"rays": N, "seed": SEED, "ray_id_offset": OFF, "image": IMAGE_N, "spectra": True},
           "fixed64_arrays": len(fixed), "fixed64_all_byte_identical": all(fixed.values()),
           "fixed64_differing": sorted(k for k, v in fixed.items() if not v),
           "f64_arrays": len([k for k in a.files if "/f64/" in k]),
           "f64_counters_equal": counters_equal, "f64_sums_max_rel_diff": worst, "f64_sums_max_rel_diff_at": worst_key,
           "f64_sums_that_differ": n_differ}
    ok = out["fixed64_all_byte_identical"] and counters_equal
    if again_path:
        a2 = np.load(again_path)
        assert sorted(a.files) == sorted(a2.files)
        eq2, worst2, key2, n2 = f64_differences(a, a2)
        out.update({"parent_again_fixed64_all_byte_identical": all(a[k].tobytes() == a2[k].tobytes() for k in fixed),
                    "parent_vs_parent_f64_counters_equal": eq2, "parent_vs_parent_f64_sums_max_rel_diff": worst2,
                    "parent_vs_parent_f64_sums_max_rel_diff_at": key2, "parent_vs_parent_f64_sums_that_differ": n2,
                    "f64_sums_within_parent_vs_parent": worst <= worst2})
        ok = ok and worst <= worst2
    text = json.dumps(out, indent=1)
    print(text)
    if json_path:
        open(json_path, "w").write(text + "\n")
    return 0 if ok else 1


def option(name):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else None


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3], option("--json"), option("--parent-again")))
