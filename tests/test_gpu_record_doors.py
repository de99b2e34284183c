"""The three record doors on ONE context, one after the other: sart_trace_records, sart_trace_records_passed[_device] and
sart_trace_columns_passed[_device] are driven by one chunk pipeline and share its streams and events, the record buffers d_rec /
d_rec2 and the pinned chunk totals.  Every other test uses one door per context; here the state one door leaves behind meets the
next door.  The reference is one single-launch traceAxionWrapper of a context of its own, taken before the chunk knob is set: it
does not pass through the pipeline.  Equality is on bytes.  No failure is injected."""
import numpy as np
import pytest

import solaraxionraytracing_amd as sa
from solaraxionraytracing_amd import _lib as L
from solaraxionraytracing_amd.raytracer import columns_from_records
from tests.conftest import make_setup

pytestmark = pytest.mark.gpu

N_BIG, N_SMALL, CHUNK = 150_001, 1_025, 40_001      # four chunks: three full, one of 29 998 rays; no multiple of 64 or 1024
SEED, OFFSET = 31, 7
COUNT_KEYS = ("n_rays", "n_passed", "n_passed_till_window", "n_hit_nickel")
SOME = sa.RayTracer.DEFAULT_COLUMNS + ("ray_id",)


class Reference:
    """Everything the doors return for the first n rays, derived on the host from the full record buffer."""

    def __init__(self, full):
        self.full = full

    def records(self, n):
        return self.full[:n]

    def counts(self, n):
        f = self.full[:n]
        return {"n_rays": n, "n_passed": int((f["passed"] != 0).sum()), "n_passed_till_window": int((f["passedTillWindow"] != 0).sum()),
                "n_hit_nickel": int((f["hitNickel"] != 0).sum())}

    def passed(self, n):
        # (rows of the byte view: a fancy-indexed copy of a structured array does not carry the padding bytes)
        f = self.full[:n]
        return f.view(np.uint8).reshape(n, 208)[f["passed"] != 0]

    def columns(self, n):
        f = self.full[:n]
        sel = f["passed"] != 0
        return columns_from_records(f[sel], L.COLUMNS, ray_ids=np.uint64(OFFSET) + np.nonzero(sel)[0].astype(np.uint64))


def same_columns(got, want, names, m=None):
    assert list(got) == sorted(set(names), key=L.COLUMNS.get)
    for c in got:
        w = want[c] if m is None else want[c][:m]
        assert got[c].dtype == L.column_dtype(c) and got[c].shape == w.shape, c
        assert got[c].tobytes() == w.tobytes(), c


def test_the_doors_one_after_the_other_on_one_context(monkeypatch):
    import torch
    monkeypatch.delenv("SART_RECORDS_CHUNK", raising=False)
    with sa.RayTracer(make_setup("cast_llnl")) as rt:
        full = rt.traceAxionWrapper(N_BIG, seed=SEED, ray_id_offset=OFFSET)      # one launch, one copy
    full.setflags(write=False)
    ref = Reference(full)
    counts_big, counts_small = ref.counts(N_BIG), ref.counts(N_SMALL)
    m = counts_big["n_passed"]
    assert 0 < m < N_BIG and 0 < counts_small["n_passed"] < N_SMALL
    passed_big, cols_big, cols_small = ref.passed(N_BIG), ref.columns(N_BIG), ref.columns(N_SMALL)
    kw = dict(seed=SEED, ray_id_offset=OFFSET)

    # the device buffers of step 9, made before anything is measured (the allocator keeps what it takes)
    d_rec = torch.full(((m + 3) * 208,), 0xAB, dtype=torch.uint8, device="cuda")
    d_col = torch.full((len(SOME), m + 3), 0x5B5B5B5B, dtype=torch.int64, device="cuda")
    d_cnt_rec = torch.full((4,), 99, dtype=torch.int64, device="cuda")
    d_cnt_col = torch.full((4,), 99, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    monkeypatch.setenv("SART_RECORDS_CHUNK", str(CHUNK))                        # read at sart_create
    with sa.RayTracer(make_setup("cast_llnl")) as rt:
        # 1. records, small: the single-chunk fast path
        assert rt.traceAxionWrapper(N_SMALL, **kw).tobytes() == ref.records(N_SMALL).tobytes()
        # 2. passed, big
        got, c = rt.traceAxionWrapperPassed(N_BIG, **kw)
        assert c == counts_big and got.tobytes() == passed_big.tobytes()
        # 3. records, big
        assert rt.traceAxionWrapper(N_BIG, **kw).tobytes() == full.tobytes()
        # 4. columns, small, all 27: one half-buffer only
        got, c = rt.trace_columns(N_SMALL, tuple(L.COLUMNS), **kw)
        assert c == counts_small
        same_columns(got, cols_small, L.COLUMNS)
        # 5. columns, big, the six default columns and the ray id: now two half-buffers
        got, c = rt.trace_columns(N_BIG, SOME, **kw)
        assert c == counts_big
        same_columns(got, cols_big, SOME)
        # 6. records, big
        assert rt.traceAxionWrapper(N_BIG, **kw).tobytes() == full.tobytes()
        torch.cuda.synchronize()
        free_after_6 = torch.cuda.mem_get_info()[0]
        # 7. passed, big, into a guarded buffer with room for a third of them
        cap = m // 3
        guard = np.zeros(cap + 5, dtype=L.AXION_DTYPE)
        guard["weights"] = -7.0
        few, c = rt.traceAxionWrapperPassed(N_BIG, capacity=cap, out=guard, **kw)
        assert c == counts_big and len(few) == cap and few.tobytes() == passed_big[:cap].tobytes()
        assert (guard[cap:]["weights"] == -7.0).all()                          # nothing behind the capacity is touched
        # 8. columns, big, the ray id alone: no staged word
        got, c = rt.trace_columns(N_BIG, ("ray_id",), **kw)
        assert c == counts_big
        same_columns(got, cols_big, ("ray_id",))
        # 9. the two device doors, big (compared below, once nothing more is to be measured)
        rt.trace_records_passed_device(rt.trace_params(N_BIG, **kw), d_rec.data_ptr(), m + 3, d_cnt_rec.data_ptr())
        d_cols, _ = rt.trace_columns_device(rt.trace_params(N_BIG, **kw), SOME, m + 3, out=d_col, counts=d_cnt_col)
        rt.synchronize()
        # 10. records, big, once more
        assert rt.traceAxionWrapper(N_BIG, **kw).tobytes() == full.tobytes()
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == free_after_6                    # no step after the sixth allocated or freed

        want_counts = [counts_big[k] for k in COUNT_KEYS]
        assert d_cnt_rec.tolist() == want_counts and d_cnt_col.tolist() == want_counts
        h_rec = d_rec.cpu().numpy()
        assert h_rec[:m * 208].tobytes() == passed_big.tobytes() and (h_rec[m * 208:] == 0xAB).all()
        for name in SOME:
            h = d_cols[name].cpu().numpy()
            assert h[:m].tobytes() == cols_big[name].tobytes(), name
            assert (h[m:].view(np.int64) == 0x5B5B5B5B).all(), name
