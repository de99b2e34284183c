"""sart_trace_columns_passed[_device]: the passed rays as selected columns, structure-of-arrays, in ray order.  The reference is
always the record path, none of which this feature touches: traceAxionWrapper's buffer filtered on `passed`, through
raytracer.columns_from_records.  Equality is on bytes."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import solaraxionraytracing_amd as sa
from solaraxionraytracing_amd import _lib as L
from solaraxionraytracing_amd.raytracer import columns_from_records
from tests.conftest import make_setup

pytestmark = pytest.mark.gpu

PHYSICS = sa.RayTracer.DEFAULT_COLUMNS                                   # the six words generateResultPlots reads
MASKS = {"physics": PHYSICS, "single": ("reflect",), "not_double": ("flags", "kinds_packed", "shellNumber", "ray_id"),
         "all": tuple(L.COLUMNS)}
COUNT_KEYS = ("n_rays", "n_passed", "n_passed_till_window", "n_hit_nickel")
GUARD = np.uint64(0xA5A5_5A5A_DEAD_BEEF)


@functools.lru_cache(maxsize=None)
def reference_of(name, n, seed, offset):
    """All 27 columns of the passed rays out of the full record buffer, and the counts; computed once per case, never changed."""
    with sa.RayTracer(make_setup(name)) as rt:
        full = rt.traceAxionWrapper(n, seed=seed, ray_id_offset=offset)
    sel = full["passed"] != 0
    counts = {"n_rays": n, "n_passed": int(sel.sum()), "n_passed_till_window": int((full["passedTillWindow"] != 0).sum()),
              "n_hit_nickel": int((full["hitNickel"] != 0).sum())}
    cols = columns_from_records(full[sel], L.COLUMNS, ray_ids=np.uint64(offset) + np.nonzero(sel)[0].astype(np.uint64))
    for a in cols.values():
        a.setflags(write=False)
    return cols, counts, np.nonzero(sel)[0]


def same_bytes(got, want, names, m=None):
    assert list(got) == sorted(set(names), key=L.COLUMNS.get)
    for c in got:
        w = want[c] if m is None else want[c][:m]
        assert got[c].dtype == L.column_dtype(c) and got[c].shape == w.shape, c
        assert got[c].tobytes() == w.tobytes(), c


@pytest.mark.parametrize("name", ["babyiaxo_xmm", "cast_llnl", "babyiaxo_xmm_gas"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025, 200_003])
def test_columns_are_the_filtered_buffer(name, n):
    want, counts, passed_at = reference_of(name, n, 17, 5)
    if n >= 1025:
        assert 0 < counts["n_passed"] < n
    with sa.RayTracer(make_setup(name)) as rt:
        for which, names in MASKS.items():
            got, c = rt.trace_columns(n, names, seed=17, ray_id_offset=5)
            assert c == counts, which
            same_bytes(got, want, names)
        ids, _ = rt.trace_columns(n, ("ray_id",), seed=17, ray_id_offset=5)
    assert ids["ray_id"].dtype == np.uint64 and ids["ray_id"].tolist() == (5 + passed_at).tolist()


@pytest.mark.parametrize("chunk", [65_536, 40_001, 1_000])
def test_ragged_chunks_small_capacity_and_guards(chunk, monkeypatch):
    """Several chunks through the two half-buffers, chunk sizes that are no multiple of the compaction's blocks.  A capacity below
    the passed rays (an odd stride) keeps the first `capacity` of every column, counts all and writes nothing behind the last
    column; a capacity above them leaves the tail of every column as it was."""
    n = 150_001
    want, counts, _ = reference_of("cast_llnl", n, 31, 7)
    monkeypatch.setenv("SART_RECORDS_CHUNK", str(chunk))
    names = PHYSICS + ("ray_id",)
    k = len(names)
    with sa.RayTracer(make_setup("cast_llnl")) as rt:
        got, c = rt.trace_columns(n, names, seed=31, ray_id_offset=7)
        assert c == counts
        same_bytes(got, want, names)
        cap = counts["n_passed"] // 3
        assert cap > 0
        buf = np.full(k * cap + 9, GUARD, dtype=np.uint64)
        few, c2 = rt.trace_columns(n, names, seed=31, ray_id_offset=7, capacity=cap, out=buf)
        assert c2 == counts
        same_bytes(few, want, names, cap)
        assert (buf[k * cap:] == GUARD).all()                              # nothing behind the last column
        roomy = counts["n_passed"] + 5
        buf = np.full(k * roomy + 9, GUARD, dtype=np.uint64)
        all_of, c3 = rt.trace_columns(n, names, seed=31, ray_id_offset=7, capacity=roomy, out=buf)
        assert c3 == counts
        same_bytes(all_of, want, names)
        assert (buf[:k * roomy].reshape(k, roomy)[:, counts["n_passed"]:] == GUARD).all() and (buf[k * roomy:] == GUARD).all()
        buf = np.full(9, GUARD, dtype=np.uint64)
        none, c4 = rt.trace_columns(n, names, seed=31, ray_id_offset=7, capacity=0, out=buf)
        assert c4 == counts and all(len(v) == 0 for v in none.values()) and (buf == GUARD).all()
        cnt = L.RecordCounts()
        p = rt.trace_params(n, 31, 7)
        assert rt.lib.sart_trace_columns_passed(rt.handle, C.byref(p), L.column_mask(names), None, 0, C.byref(cnt)) == 0   # NULL with capacity 0
        assert {f: int(getattr(cnt, f)) for f in COUNT_KEYS} == counts


def test_device_form_appends_over_launches():
    """Two launches with `accumulate` into one buffer = one reference over both ranges; 3 Mi rays cross the 2^20 chunk inside a
    call.  A buffer for half of the passed rays keeps the first half of every column and the rest of the buffer as it was."""
    import torch
    n1, n2 = 1_300_000, 1_845_729
    names = tuple(L.COLUMNS)
    k = len(names)
    want, counts, _ = reference_of("babyiaxo_xmm", n1 + n2, 9, 11)
    m = counts["n_passed"]
    with sa.RayTracer(make_setup("babyiaxo_xmm")) as rt:
        cap = m + 10
        out = torch.full((k, cap), 0x5B5B5B5B, dtype=torch.int64, device="cuda")
        cnt = torch.full((4,), 99, dtype=torch.int64, device="cuda")
        cols, cnt_out = rt.trace_columns_device(rt.trace_params(n1, seed=9, ray_id_offset=11), names, cap, out=out, counts=cnt)
        rt.trace_columns_device(rt.trace_params(n2, seed=9, ray_id_offset=11 + n1, accumulate=True), names, cap, out=out, counts=cnt)
        rt.synchronize()
        assert cnt_out.data_ptr() == cnt.data_ptr() and cnt.tolist() == [counts[f] for f in COUNT_KEYS]
        for c in names:
            assert cols[c].data_ptr() == out[L.COLUMNS[c]].data_ptr() and cols[c].shape == (cap,)      # zero-copy views, in bit order
            assert cols[c].dtype == (torch.float64 if L.column_dtype(c) == np.float64 else torch.int64)
            assert cols[c][:m].cpu().numpy().tobytes() == want[c].tobytes(), c
        assert (out[:, m:] == 0x5B5B5B5B).all().item()
        half = m // 2
        small = torch.full((k * half + 3,), 0x5B5B5B5B, dtype=torch.int64, device="cuda")
        cols, cnt2 = rt.trace_columns_device(rt.trace_params(n1 + n2, seed=9, ray_id_offset=11), names, half, out=small)
        rt.synchronize()
        assert cnt2.tolist() == [counts[f] for f in COUNT_KEYS]
        for c in names:
            assert cols[c].cpu().numpy().tobytes() == want[c][:half].tobytes(), c
        assert (small[k * half:] == 0x5B5B5B5B).all().item()
        # a buffer the call makes itself, on the context's device
        cols, cnt3 = rt.trace_columns_device(rt.trace_params(70_000, seed=9, ray_id_offset=11), PHYSICS, 70_000)
        rt.synchronize()
        m3 = int(cnt3[1])
        assert 0 < m3 == int((want["ray_id"] < 11 + 70_000).sum()) and cols["weights"].device.type == "cuda"
        for c in PHYSICS:
            assert cols[c][:m3].cpu().numpy().tobytes() == want[c][:m3].tobytes(), c


def test_no_ray_passes_and_no_rays():
    full = make_setup("babyiaxo_xmm")
    full.setup.chip_x_max = full.setup.chip_y_max = 1e-6      # a chip nobody hits
    with sa.RayTracer(full) as rt:
        buf = np.full(7 * 50_000 + 3, GUARD, dtype=np.uint64)
        got, c = rt.trace_columns(50_000, PHYSICS + ("ray_id",), seed=3, out=buf)
        assert all(len(v) == 0 for v in got.values()) and len(got) == 7 and (buf == GUARD).all()
        assert c["n_passed"] == 0 and c["n_rays"] == 50_000 and c["n_passed_till_window"] > 0
        got, c = rt.trace_columns(0, PHYSICS)
        assert all(len(v) == 0 for v in got.values()) and c == dict.fromkeys(COUNT_KEYS, 0)


def test_failure_inside_the_pipeline_leaves_through_the_synchronised_exit(monkeypatch):
    """SART_RECORDS_FAIL_CHUNK injects a software error in the third chunk (no GPU fault): the call returns it after both streams
    have drained, and a new context works."""
    monkeypatch.setenv("SART_RECORDS_CHUNK", "30000")
    monkeypatch.setenv("SART_RECORDS_FAIL_CHUNK", "3")
    with sa.RayTracer(make_setup("cast_llnl")) as rt:
        with pytest.raises(L.SartError, match="SART_RECORDS_FAIL_CHUNK"):
            rt.trace_columns(200_000, PHYSICS, seed=1)
    monkeypatch.delenv("SART_RECORDS_FAIL_CHUNK")
    with sa.RayTracer(make_setup("cast_llnl")) as rt:
        got, c = rt.trace_columns(200_000, PHYSICS, seed=1)
        assert c["n_passed"] == len(got["weights"]) > 100_000


def test_invalid_arguments_leave_the_context_as_it_was():
    import torch
    names = PHYSICS + ("ray_id",)
    mask = L.column_mask(names)
    want, counts, _ = reference_of("cast_llnl", 1025, 17, 5)
    with sa.RayTracer(make_setup("cast_llnl")) as rt:
        before, _ = rt.trace_columns(1025, names, seed=17, ray_id_offset=5)
        p = rt.trace_params(1025, 17, 5)
        cnt = L.RecordCounts()
        buf = np.full(7 * 1025, GUARD, dtype=np.uint64)
        host = lambda *a: rt.lib.sart_trace_columns_passed(*a)
        ptr = buf.ctypes.data_as(C.c_void_p)
        bad = L.SART_ERR_INVALID_ARGUMENT
        assert host(rt.handle, C.byref(p), 0, ptr, 1025, C.byref(cnt)) == bad                       # no column
        assert host(rt.handle, C.byref(p), 1 << 27, ptr, 1025, C.byref(cnt)) == bad                 # a bit that names no column
        assert host(rt.handle, C.byref(p), mask | (1 << 31), ptr, 1025, C.byref(cnt)) == bad
        assert host(None, C.byref(p), mask, ptr, 1025, C.byref(cnt)) == bad
        assert host(rt.handle, None, mask, ptr, 1025, C.byref(cnt)) == bad
        assert host(rt.handle, C.byref(p), mask, None, 1025, C.byref(cnt)) == bad                   # NULL columns with room asked for
        assert host(rt.handle, C.byref(p), mask, ptr, 1025, None) == bad
        assert host(rt.handle, C.byref(p), mask, ptr, 1 << 63, C.byref(cnt)) == bad                 # 7 x 2^63 slots
        assert host(rt.handle, C.byref(p), mask, ptr, (1 << 64) // 7 + 1, C.byref(cnt)) == bad
        assert (buf == GUARD).all()
        out = torch.full((7 * 1025,), 0x5B, dtype=torch.int64, device="cuda")
        dcnt = torch.full((4,), 99, dtype=torch.int64, device="cuda")
        dev = lambda *a: rt.lib.sart_trace_columns_passed_device(*a)
        optr, cptr = C.c_void_p(out.data_ptr()), C.c_void_p(dcnt.data_ptr())
        assert dev(rt.handle, C.byref(p), 0, optr, 1025, cptr) == bad
        assert dev(rt.handle, C.byref(p), 1 << 27, optr, 1025, cptr) == bad
        assert dev(None, C.byref(p), mask, optr, 1025, cptr) == bad
        assert dev(rt.handle, None, mask, optr, 1025, cptr) == bad
        assert dev(rt.handle, C.byref(p), mask, None, 1025, cptr) == bad
        assert dev(rt.handle, C.byref(p), mask, optr, 1025, None) == bad
        assert dev(rt.handle, C.byref(p), mask, optr, 1 << 63, cptr) == bad
        rt.synchronize()
        assert (out == 0x5B).all().item() and dcnt.tolist() == [99] * 4
        after, c = rt.trace_columns(1025, names, seed=17, ray_id_offset=5)
        assert c == counts
        same_bytes(after, want, names)
        same_bytes(after, before, names)


def test_column_scratch_only_grows_and_can_be_released():
    import torch
    n = 300_000
    with sa.RayTracer(make_setup("babyiaxo_xmm")) as rt:
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        big, cb = rt.trace_columns(n, PHYSICS, seed=4)
        after_big = torch.cuda.mem_get_info()[0]
        assert free0 - after_big >= n * (6 * 8 + 4)                          # at least the staged words and flags
        small, cs = rt.trace_columns(40_000, PHYSICS, seed=4)
        again, ca = rt.trace_columns(n, PHYSICS, seed=4)
        assert torch.cuda.mem_get_info()[0] == after_big                     # nothing freed, nothing allocated in between
        assert ca == cb
        same_bytes(again, big, PHYSICS)
        same_bytes(small, big, PHYSICS, cs["n_passed"])
        L.check(rt.lib.sart_release_scratch(rt.handle))
        assert torch.cuda.mem_get_info()[0] >= after_big + n * (6 * 8 + 4)   # handed back
        once_more, cm = rt.trace_columns(n, PHYSICS, seed=4)
        assert cm == cb
        same_bytes(once_more, big, PHYSICS)


def test_events_file_of_the_command_line(tmp_path):
    from solaraxionraytracing_amd.__main__ import EVENT_COLUMNS, main
    path = tmp_path / "events.npz"
    assert main(["--rays", "200000", "--seed", "11", "--outpath", str(tmp_path / "out"), "--events", str(path)]) == 0
    with sa.RayTracer(sa.initFullSetup()) as rt:
        want, counts = rt.trace_columns(200_000, EVENT_COLUMNS, seed=11)
    assert 0 < counts["n_passed"] < 200_000
    with np.load(path) as z:
        assert sorted(z.files) == sorted(EVENT_COLUMNS + COUNT_KEYS)
        for c in EVENT_COLUMNS:
            assert z[c].dtype == L.column_dtype(c) and z[c].tobytes() == want[c].tobytes(), c
        assert {f: int(z[f]) for f in COUNT_KEYS} == counts
