#!/usr/bin/env python3
"""Outputs of the two breakdown entries of one build, for a parent / new comparison of two builds on the same box:

  SART_LIBSART=<parent .so> python tools/breakdown_outputs.py dump parent.npz
  python tools/breakdown_outputs.py dump new.npz
  python tools/breakdown_outputs.py compare parent.npz new.npz [--json OUT]

dump: the five setups of tests/test_gpu_shells.py at that test's shape (400 000 rays, seed 7, offset 13, image 256 x 256 with
spectra).  FIXED64: the raw int64 accumulator and shell block of a shells launch, the raw accumulator and channel block of a channels
launch at T = 3 and T = 8 (random fractions; not for the X-ray test source, which has no emission channels).  f64: the scalars and the
rows of the same launches.
compare: every FIXED64 array byte for byte; in f64 every counter equal and the largest relative difference of the sums.  Exit status
1 unless all of that holds."""
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
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays; build", L.build_id())


def compare(a_path, b_path, json_path):
    a, b = np.load(a_path), np.load(b_path)
    assert sorted(a.files) == sorted(b.files)
    fixed = {k: bool(a[k].tobytes() == b[k].tobytes()) for k in a.files if "/fixed64/" in k}
    counters_equal, worst, worst_key = True, 0.0, None
    for k in (k for k in a.files if "/f64/" in k):
        kind = k.split("/")[2]
        names = L.ACC if k.endswith("/scalars") else L.SHELL if kind == "shells" else L.CHAN
        x, y = a[k].reshape(-1, a[k].shape[-1]), b[k].reshape(-1, b[k].shape[-1])
        for key, slot in names.items():
            if key.startswith("N_"):
                counters_equal &= bool(np.array_equal(x[:, slot], y[:, slot]))
            else:
                d = np.abs(x[:, slot] - y[:, slot])
                rel = float(np.max(np.where(x[:, slot] != 0, d / np.where(x[:, slot] != 0, np.abs(x[:, slot]), 1.0), d)))
                if rel > worst:
                    worst, worst_key = rel, "%s %s" % (k, key)
    out = {"shape": {"rays": N, "seed": SEED, "ray_id_offset": OFF, "image": IMAGE_N, "spectra": True},
           "fixed64_arrays": len(fixed), "fixed64_all_byte_identical": all(fixed.values()),
           "fixed64_differing": sorted(k for k, v in fixed.items() if not v),
           "f64_counters_equal": counters_equal, "f64_sums_max_rel_diff": worst, "f64_sums_max_rel_diff_at": worst_key}
    text = json.dumps(out, indent=1)
    print(text)
    if json_path:
        open(json_path, "w").write(text + "\n")
    return 0 if out["fixed64_all_byte_identical"] and counters_equal else 1


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[5] if len(sys.argv) > 5 and sys.argv[4] == "--json" else None))
