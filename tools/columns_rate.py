#!/usr/bin/env python3
"""Rate of sart_trace_columns_passed[_device] (the passed rays as selected columns) beside the record interface it relieves,
sart_trace_records_passed[_device], in one process on the same context: rays per second and bytes per traced ray for 1, 6 and 26
columns - host form into mapped pages and into a fresh buffer, device form alone - and the time of the stage kernel alone
(sart_enable_kernel_timing) beside that of the record kernel.  Every shape is warmed first; the compared forms alternate inside
each of three rounds; the table gives the median and the spread (max - min) / median.

  python tools/columns_rate.py [--rays 2e7] [--out out/columns_rate]      (writes .json and .txt)"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=float, default=2e7)
    ap.add_argument("--out", default="out/columns_rate")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    n = int(args.rays)
    import torch
    import solaraxionraytracing_amd as sa
    from solaraxionraytracing_amd import _lib as L
    full = sa.initFullSetup()
    words = [c for c in sorted(L.COLUMNS, key=L.COLUMNS.get) if c != "ray_id"]
    shapes = {1: ("weights",), 6: sa.RayTracer.DEFAULT_COLUMNS, 26: tuple(words)}

    with sa.RayTracer(full) as rt:
        _, c = rt.trace_columns(n, ("weights",), seed=5, capacity=0)
        n_passed = c["n_passed"]
        cap = int(n_passed * 1.02)
        p = rt.trace_params(n, seed=5)
        cnt = torch.zeros(4, dtype=torch.int64, device="cuda:0")
        rec_host = np.zeros(cap, dtype=L.AXION_DTYPE)                     # mapped: every page written
        rec_dev = torch.empty(cap * 208, dtype=torch.uint8, device="cuda:0")
        col_host = {k: np.zeros(k * cap, dtype=np.uint64) for k in shapes}
        col_dev = {k: torch.empty((k, cap), dtype=torch.int64, device="cuda:0") for k in shapes}

        def wall(f):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            rt.synchronize()
            return time.perf_counter() - t0

        def fresh_records():
            buf = np.empty(cap, dtype=L.AXION_DTYPE)                      # no page of it exists yet
            return wall(lambda: rt.traceAxionWrapperPassed(n, seed=5, out=buf))

        def fresh_columns(k):
            buf = np.empty(k * cap, dtype=np.uint64)
            return wall(lambda: rt.trace_columns(n, shapes[k], seed=5, capacity=cap, out=buf))

        forms = {"records host mapped": lambda: wall(lambda: rt.traceAxionWrapperPassed(n, seed=5, out=rec_host)),
                 "records host fresh": fresh_records,
                 "records device": lambda: wall(lambda: rt.trace_records_passed_device(p, rec_dev.data_ptr(), cap, cnt.data_ptr()))}
        for k in shapes:
            forms["columns %d host mapped" % k] = lambda k=k: wall(lambda: rt.trace_columns(n, shapes[k], seed=5, capacity=cap, out=col_host[k]))
            forms["columns %d host fresh" % k] = lambda k=k: fresh_columns(k)
            forms["columns %d device" % k] = lambda k=k: wall(lambda: rt.trace_columns_device(p, shapes[k], cap, out=col_dev[k], counts=cnt))
        for f in forms.values():                                          # warm every shape: scratch, streams, events, pages
            f()
        times = {label: [] for label in forms}
        for _ in range(args.rounds):
            for label, f in forms.items():                                # the compared forms alternate
                times[label].append(f())
        # the same rays in both interfaces (first 20 000 passed rays, the six default columns)
        got, _ = rt.trace_columns(n, shapes[6], seed=5, capacity=cap, out=col_host[6])
        rec, _ = rt.traceAxionWrapperPassed(n, seed=5, out=rec_host)
        for c in shapes[6]:
            assert got[c][:20_000].tobytes() == np.ascontiguousarray(rec[c][:20_000]).tobytes(), c
        # kernel time alone: the record kernel, and the stage kernel per shape (events around that launch only)
        kernel_ms = {}
        rt.enable_kernel_timing(True)
        for _ in range(args.rounds):
            rt.trace_records_passed_device(p, rec_dev.data_ptr(), cap, cnt.data_ptr())
            kernel_ms.setdefault("records", []).append(rt.kernel_timing()[0])
            for k in shapes:
                rt.trace_columns_device(p, shapes[k], cap, out=col_dev[k], counts=cnt)
                kernel_ms.setdefault("columns %d" % k, []).append(rt.kernel_timing()[0])
        rt.enable_kernel_timing(False)

    def row(ts, bytes_per_passed):
        med = statistics.median(ts)
        return {"seconds": ts, "median_s": med, "spread": (max(ts) - min(ts)) / med, "rays_per_s": n / med,
                "bytes_per_traced_ray": bytes_per_passed * n_passed / n}

    res = {"rays": n, "n_passed": n_passed, "passed_fraction": n_passed / n, "capacity": cap, "rounds": args.rounds, "forms": {},
           "kernel_alone": {}}
    for label, ts in times.items():
        k = int(label.split()[1]) if label.startswith("columns") else 26
        res["forms"][label] = row(ts, 8 * k)
    for label, ms in kernel_ms.items():
        med = statistics.median(ms)
        res["kernel_alone"][label] = {"ms": ms, "median_ms": med, "spread": (max(ms) - min(ms)) / med, "rays_per_s": n / (med / 1e3)}
    F = res["forms"]
    res["host_mapped_6_columns_over_records"] = F["columns 6 host mapped"]["rays_per_s"] / F["records host mapped"]["rays_per_s"]
    res["device_6_columns_over_records"] = F["columns 6 device"]["rays_per_s"] / F["records device"]["rays_per_s"]
    lines = ["%d rays, %d passed (%.4f), buffers of %d rays, median of %d (spread = (max - min) / median)"
             % (n, n_passed, n_passed / n, cap, args.rounds), "",
             "%-26s %12s %8s %10s" % ("form", "rays/s", "spread", "B/ray")]
    for label, r in F.items():
        lines.append("%-26s %12.4e %7.1f%% %10.2f" % (label, r["rays_per_s"], 100 * r["spread"], r["bytes_per_traced_ray"]))
    lines += ["", "%-26s %12s %8s %10s" % ("kernel alone", "rays/s", "spread", "ms")]
    for label, r in res["kernel_alone"].items():
        lines.append("%-26s %12.4e %7.1f%% %10.3f" % (label, r["rays_per_s"], 100 * r["spread"], r["median_ms"]))
    lines += ["", "host form into mapped pages, 6 columns / records: %.2fx" % res["host_mapped_6_columns_over_records"],
              "device form, 6 columns / records: %.2fx" % res["device_6_columns_over_records"]]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out + ".json", "w"), indent=1)
    open(args.out + ".txt", "w").write(text)


if __name__ == "__main__":
    main()
