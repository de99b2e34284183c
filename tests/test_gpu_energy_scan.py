"""Fused energy scan of the X-ray test source (include/sart.h: sart_trace_energy_scan) on the MI355X box.

With the test source the energy is a constant of the setup (raytracer.nim:1771) that enters a ray's weight only.  The scan
traces every ray once and weighs it at K energies.  Demanded here, per energy:
  * SART_ACCUM_FIXED64: the raw integers equal those of a single launch after sart_set_setup with that test_energy, on the same
    ray ids - bit for bit, for both generic kernel variants, vacuum and gas, one and four coatings, any split of the energies;
  * SART_ACCUM_F64: the flux equals the single launch to 1e-12 (summation order), the counters exactly;
  * the flux equals the CPU oracle with that energy to 1e-6;
  * the CAST / LLNL effective-area curve in one call equals the host loop it replaces and meets the DTU thesis curve."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import solaraxionraytracing_amd as sa
from solaraxionraytracing_amd import _lib as L, tables

from tests.conftest import SMALL, make_setup

pytestmark = pytest.mark.gpu

N_IMG = 256 * 256
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO40 = 2 ** L.FIXED_LIMB_BITS


def energies(k):
    """k energies [keV]: tiny (window and gas transmission underflow: no ray passes), below the reflectivity grid (0.03 - 15 keV),
    on its first node, above it, a duplicate pair, then a spread."""
    e = np.concatenate([[1e-300, 0.01, 0.03, 20.0, 1.5, 1.5], np.linspace(0.3, 12.0, max(0, k - 6))])
    return np.ascontiguousarray(e[:k])


def xray_source(parallel=1, radius=21.5, energy=1.0):
    src = L.TestSourceConfig()
    src.active, src.parallel = 1, parallel
    src.energy, src.distance, src.radius, src.activity = energy, 100.0, radius, 1.0
    src.offAxisUp = src.offAxisLeft = src.lengthCol = 0.0
    return src


def setup_of(name):
    if name == "cast_llnl_gold":
        return sa.initFullSetup(L.ES_CAST, L.DK_INGRID2018, L.SK_VACUUM, L.TK_LLNL, flags=L.CF_XRAY_TEST, source_cfg=xray_source(),
                                reflectivity="gold", **SMALL)
    if name == "cast_llnl":   # four coatings
        return sa.initFullSetup(L.ES_CAST, L.DK_INGRID2018, L.SK_VACUUM, L.TK_LLNL, flags=L.CF_XRAY_TEST, source_cfg=xray_source(), **SMALL)
    if name == "babyiaxo_xmm_xray":
        return make_setup("babyiaxo_xmm_xray")
    if name == "babyiaxo_xmm_xray_rot":
        full = make_setup("babyiaxo_xmm_xray")
        full.setup.telescope_turned_x_deg, full.setup.telescope_turned_y_deg = 0.01, 0.03
        return full
    if name == "babyiaxo_xmm_xray_gas":   # energy-dependent q, Gamma and pipe / magnet absorption in the conversion probability
        return sa.initFullSetup(stage=L.SK_GAS, flags=L.CF_XRAY_TEST, **SMALL)
    raise KeyError(name)


def get_setup(rt):
    s = L.Setup()
    L.check(rt.lib.sart_get_setup(rt.handle, C.byref(s)))
    return s


def set_test_energy(rt, e):
    s = get_setup(rt)
    s.test_energy = float(e)
    L.check(rt.lib.sart_set_setup(rt.handle, C.byref(s)))


def raw_single(rt, torch, e, n, seed, off=0, flags=None):
    """Scalars of the raw FIXED64 accumulator of one single launch at test energy e (the context's energy is put back)."""
    e0 = get_setup(rt).test_energy
    acc = torch.zeros(sa.accumulator_len(256), dtype=torch.int64, device="cuda")
    set_test_energy(rt, e)
    try:
        p = rt.trace_params(n, seed=seed, ray_id_offset=off, flags=flags, accumulate=False)
        rt.trace_histogram_device(p, acc.data_ptr())
        rt.synchronize()
    finally:
        set_test_energy(rt, e0)
    return acc.cpu().numpy()[N_IMG:]


def raw_scan(rt, torch, es, pieces, seed, flags=None):
    acc = torch.zeros(L.energy_scan_len(len(es)), dtype=torch.int64, device="cuda")
    for lo, hi in pieces:
        p = rt.trace_params(hi - lo, seed=seed, ray_id_offset=lo, flags=flags, accumulate=True)
        rt.trace_energy_scan_device(p, es, acc.data_ptr())
    rt.synchronize()
    return acc.cpu().numpy().reshape(len(es) + 1, L.ESCAN_ROW)


def assert_row_equals_single(row, shared, single, k):
    A = L.ACC
    assert row[L.ESCAN["SUM_WEIGHTS"]] == single[A["SUM_WEIGHTS"]], k
    assert row[L.ESCAN_HI["SUM_WEIGHTS"]] == single[L.ACC_HI["SUM_WEIGHTS"]], k
    assert row[L.ESCAN["SUM_WEIGHTS_SQ"]] == single[A["SUM_WEIGHTS_SQ"]], k
    assert row[L.ESCAN_HI["SUM_WEIGHTS_SQ"]] == single[L.ACC_HI["SUM_WEIGHTS_SQ"]], k
    assert row[L.ESCAN["N_PASSED"]] == single[A["N_PASSED"]], k
    assert row[L.ESCAN["N_PASSED_TILL_WINDOW"]] == single[A["N_PASSED_TILL_WINDOW"]], k
    for key in ("N_RAYS", "N_REACHED_TELESCOPE", "N_SHELL_SELECTED", "N_HIT_NICKEL"):
        assert shared[L.ESCAN_SHARED[key]] == single[A[key]], (k, key)


CASES = [("cast_llnl_gold", 32), ("cast_llnl", 7), ("babyiaxo_xmm_xray", 33), ("babyiaxo_xmm_xray_rot", 7), ("babyiaxo_xmm_xray_gas", 7),
         ("cast_llnl_gold", 1)]


@pytest.mark.parametrize("name,k", CASES)
def test_fixed64_scan_equals_single_launches_bit_for_bit(name, k):
    import torch
    full = setup_of(name)
    es = energies(k)
    n, seed = 200_000, 11
    with sa.RayTracer(full) as rt:
        rt.set_accumulation_mode("fixed64")
        before = bytes(get_setup(rt))
        scan = raw_scan(rt, torch, es, [(0, n)], seed)
        assert bytes(get_setup(rt)) == before                       # the scan does not modify the setup
        for i, e in enumerate(es):
            assert_row_equals_single(scan[i], scan[k], raw_single(rt, torch, e, n, seed), i)
    assert scan[k][L.ESCAN_SHARED["N_RAYS"]] == n
    if k > 1 and "gas" not in name:   # (gas stage: q = |m_gamma^2 - m_a^2| / 2E overflows at 1e-300 keV and the weight is NaN - in the single launch too)
        assert scan[0][L.ESCAN["N_PASSED"]] == 0                    # 1e-300 keV: window x gas transmission underflows
    if k > 1:
        assert (scan[4] == scan[5]).all()                           # duplicate energies
        assert scan[2][L.ESCAN["N_PASSED"]] > 0 and scan[3][L.ESCAN["N_PASSED"]] > 0


def test_fixed64_scan_of_99_energies_in_balanced_groups():
    """99 energies = 25 + 25 + 25 + 24 per launch: every group equals its single launches; the finalized scan equals the
    finalized single launches."""
    import torch
    full = setup_of("babyiaxo_xmm_xray")
    es = energies(99)
    n, seed = 100_000, 3
    with sa.RayTracer(full) as rt:
        rt.set_accumulation_mode("fixed64")
        scan = raw_scan(rt, torch, es, [(0, n)], seed)
        for i in list(range(0, 99, 7)) + [24, 25, 49, 50, 74, 75, 98]:
            assert_row_equals_single(scan[i], scan[99], raw_single(rt, torch, es[i], n, seed), i)
        per_e, shared = rt.trace_energy_scan(es, n, seed=seed)
        for i in (0, 30, 60, 98):
            set_test_energy(rt, es[i])
            _, s = rt.trace_histogram(n, seed=seed)
            assert per_e["SUM_WEIGHTS"][i] == s["SUM_WEIGHTS"] and per_e["N_PASSED"][i] == s["N_PASSED"], i
        assert shared["N_RAYS"] == n


@pytest.mark.parametrize("name", ["cast_llnl_gold", "babyiaxo_xmm_xray_gas", "babyiaxo_xmm_xray_rot"])
def test_f64_scan_equals_single_launches(name):
    full = setup_of(name)
    es = energies(9)
    n, seed = 200_000, 5
    with sa.RayTracer(full) as rt:
        per_e, shared = rt.trace_energy_scan(es, n, seed=seed)
        e0 = get_setup(rt).test_energy
        for i, e in enumerate(es):
            set_test_energy(rt, e)
            _, s = rt.trace_histogram(n, seed=seed)
            if np.isnan(s["SUM_WEIGHTS"]):   # (1e-300 keV in the gas stage: NaN weights, the single launch's as well)
                assert np.isnan(per_e["SUM_WEIGHTS"][i]), i
            else:
                assert per_e["SUM_WEIGHTS"][i] == pytest.approx(s["SUM_WEIGHTS"], rel=1e-12, abs=1e-300), i
            assert per_e["N_PASSED"][i] == s["N_PASSED"] and per_e["N_PASSED_TILL_WINDOW"][i] == s["N_PASSED_TILL_WINDOW"], i
            for key in ("N_RAYS", "N_REACHED_TELESCOPE", "N_SHELL_SELECTED", "N_HIT_NICKEL"):
                assert shared[key] == s[key], key
        set_test_energy(rt, e0)


def test_sharded_rays_give_the_same_integers():
    import torch
    full = setup_of("cast_llnl")
    es = energies(7)
    n, seed = 300_000, 8
    with sa.RayTracer(full) as rt:
        rt.set_accumulation_mode("fixed64")
        whole = raw_scan(rt, torch, es, [(0, n)], seed)
        pieces = raw_scan(rt, torch, es, [(0, 77_777), (77_777, 200_001), (200_001, n)], seed)
        lo = raw_scan(rt, torch, es, [(0, n // 2)], seed)
        hi = raw_scan(rt, torch, es, [(n // 2, n)], seed)
    assert (pieces == whole).all()
    summed = lo.astype(object) + hi.astype(object)
    value = lambda r, s: int(r[L.ESCAN_HI[s]]) * TWO40 + int(r[L.ESCAN[s]])
    for i in range(len(es)):
        for s in ("SUM_WEIGHTS", "SUM_WEIGHTS_SQ"):
            assert value(summed[i], s) == value(whole[i], s), (i, s)
        for s in ("N_PASSED", "N_PASSED_TILL_WINDOW"):
            assert summed[i][L.ESCAN[s]] == whole[i][L.ESCAN[s]]
    assert (summed[len(es)] == whole[len(es)]).all()


@pytest.mark.parametrize("name", ["cast_llnl_gold", "babyiaxo_xmm_xray_gas"])
def test_scan_matches_the_oracle_per_energy(name):
    from oracle.oracle import Oracle
    full = setup_of(name)
    es = np.array([0.5, 1.5, 3.0, 6.0, 9.0])
    n, seed = 200_000, 4
    with sa.RayTracer(full) as rt:
        per_e, shared = rt.trace_energy_scan(es, n, seed=seed)
    o = Oracle(full)
    for i, e in enumerate(es):
        s = full.setup.copy()
        s.test_energy = float(e)
        want = o.trace_histogram(n, seed=seed, setup=s)[1]
        assert per_e["N_PASSED"][i] == want["N_PASSED"], (i, e)
        assert per_e["SUM_WEIGHTS"][i] == pytest.approx(want["SUM_WEIGHTS"], rel=1e-6), (i, e)
        for key in ("N_REACHED_TELESCOPE", "N_SHELL_SELECTED", "N_HIT_NICKEL"):
            assert shared[key] == want[key], key


DTU_FLAGS = L.CF_XRAY_TEST | L.CF_IGNORE_DET_WINDOW | L.CF_IGNORE_GAS_ABS | L.CF_IGNORE_CONV_PROB
DTU_ENERGIES = (0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 5.0, 7.0, 9.0)


def test_dtu_effective_area_curve_in_one_call():
    """tests/test_reference_data.py's host loop (a full trace per energy) as ONE scan of 0.3 - 10 keV in 0.1 keV steps: the same
    numbers at its nine energies (bit for bit in FIXED64, 1e-12 in F64), and its tolerances against the DTU thesis curve."""
    import torch
    es = np.round(np.arange(0.3, 10.0 + 1e-9, 0.1), 10)
    full = sa.initFullSetup(L.ES_CAST, L.DK_INGRID2018, L.SK_VACUUM, L.TK_LLNL, flags=DTU_FLAGS, source_cfg=xray_source(), reflectivity="gold")
    n, seed = 1_000_000, 4
    idx = [int(np.argmin(np.abs(es - e))) for e in DTU_ENERGIES]
    assert all(es[i] == e for i, e in zip(idx, DTU_ENERGIES))
    with sa.RayTracer(full) as rt:
        res = sa.performEnergyScan(rt, es, n, seed=seed, flags=DTU_FLAGS)
        for i in idx:                                                       # F64: the host loop's numbers
            set_test_energy(rt, es[i])
            _, s = rt.trace_histogram(n, seed=seed, flags=DTU_FLAGS)
            assert res["sum_weights"][i] == pytest.approx(s["SUM_WEIGHTS"], rel=1e-12)
            assert res["n_passed"][i] == s["N_PASSED"]
        rt.set_accumulation_mode("fixed64")
        scan = raw_scan(rt, torch, es, [(0, n)], seed, DTU_FLAGS)
        for i in idx:
            assert_row_equals_single(scan[i], scan[len(es)], raw_single(rt, torch, es[i], n, seed, flags=DTU_FLAGS), i)
    area = res["effective_area_cm2"]
    assert area is not None and np.allclose(area, np.pi * 2.15 ** 2 * res["sum_weights"] / n, rtol=1e-14)
    assert np.allclose(res["n_passed"] / n, 0.921, atol=0.005)             # geometric throughput of the bore, at every energy
    e_ref, a_ref = tables.llnl_effective_area()
    got = {e: area[i] for e, i in zip(DTU_ENERGIES, idx)}
    ratio = {e: got[e] / np.interp(e, e_ref, a_ref) for e in got}
    for e in (0.5, 1.0, 1.5, 2.0, 4.0, 5.0):
        assert abs(ratio[e] - 1.0) < 0.12, (e, got[e], ratio[e])
    assert 0.55 < ratio[3.0] < 0.8, ratio
    assert ratio[7.0] < 0.7 and ratio[9.0] < 0.4, ratio
    vals = [got[e] for e in (2.0, 5.0, 7.0, 9.0)]
    assert all(a > b for a, b in zip(vals, vals[1:]))


def test_invalid_arguments_leave_the_context_unchanged():
    import torch
    es = energies(5)
    n, seed = 100_000, 2
    with sa.RayTracer(make_setup("babyiaxo_xmm")) as rt:      # the solar source: no energy scan
        out = np.zeros(L.energy_scan_len(5))
        p = rt.trace_params(n, seed=seed)
        before = bytes(get_setup(rt))
        assert rt.lib.sart_trace_energy_scan(rt.handle, C.byref(p), L.as_dp(es), 5, L.as_dp(out)) == L.SART_ERR_INVALID_ARGUMENT
        assert bytes(get_setup(rt)) == before
    full = setup_of("babyiaxo_xmm_xray")
    with sa.RayTracer(full) as rt:
        rt.set_accumulation_mode("fixed64")
        fresh = raw_single(rt, torch, 2.0, n, seed)
    with sa.RayTracer(full) as rt:
        rt.set_accumulation_mode("fixed64")
        before = bytes(get_setup(rt))
        out = np.zeros(L.energy_scan_len(5))
        p = rt.trace_params(n, seed=seed)
        lib, h = rt.lib, rt.handle
        E = L.SART_ERR_INVALID_ARGUMENT
        assert lib.sart_trace_energy_scan(h, C.byref(p), L.as_dp(es), 0, L.as_dp(out)) == E
        for bad in (np.nan, np.inf, -np.inf, 0.0, -1.0):
            b = es.copy()
            b[2] = bad
            assert lib.sart_trace_energy_scan(h, C.byref(p), L.as_dp(b), 5, L.as_dp(out)) == E, bad
            assert lib.sart_trace_energy_scan_device(h, C.byref(p), L.as_dp(b), 5, C.c_void_p(out.ctypes.data)) == E, bad
        assert lib.sart_trace_energy_scan(h, None, L.as_dp(es), 5, L.as_dp(out)) == E
        assert lib.sart_trace_energy_scan(h, C.byref(p), None, 5, L.as_dp(out)) == E
        assert lib.sart_trace_energy_scan(h, C.byref(p), L.as_dp(es), 5, None) == E
        assert lib.sart_trace_energy_scan_device(h, C.byref(p), L.as_dp(es), 5, None) == E
        assert lib.sart_finalize_energy_scan_device(h, C.byref(p), L.as_dp(es), 5, None, None) == E
        assert lib.sart_trace_energy_scan(None, C.byref(p), L.as_dp(es), 5, L.as_dp(out)) == E
        assert bytes(get_setup(rt)) == before
        rt.trace_energy_scan(np.linspace(0.5, 12.0, 40), n, seed=seed)     # a successful scan (two groups)
        assert bytes(get_setup(rt)) == before
        assert (raw_single(rt, torch, 2.0, n, seed) == fresh).all()       # its tables leak into nothing that follows


def test_accumulate_and_finalize_device():
    import torch
    full = setup_of("cast_llnl_gold")
    es = energies(7)
    n, seed = 100_000, 9
    with sa.RayTracer(full) as rt:
        rt.set_accumulation_mode("fixed64")
        acc = torch.full((L.energy_scan_len(7),), 12345, dtype=torch.int64, device="cuda")
        rt.trace_energy_scan_device(rt.trace_params(n, seed=seed, accumulate=False), es, acc.data_ptr())   # accumulate 0 zeroes first
        out = torch.zeros(L.energy_scan_len(7), dtype=torch.float64, device="cuda")
        rt.finalize_energy_scan_device(rt.trace_params(n, seed=seed), es, acc.data_ptr(), out.data_ptr())
        rt.synchronize()
        per_e, shared = L.split_energy_scan(out.cpu().numpy(), 7)
        blocking, bshared = rt.trace_energy_scan(es, n, seed=seed)
    for key in blocking:
        assert np.array_equal(per_e[key], blocking[key], equal_nan=True), key
    assert shared == bshared and shared["N_RAYS"] == n


def test_cli_energy_scan_matches_perform_energy_scan(tmp_path):
    n, seed = 200_000, 5
    r = subprocess.run([sys.executable, "-m", "solaraxionraytracing_amd", "--xrayTest", "--energyScanMin", "1", "--energyScanMax", "8",
                        "--numEnergyScanPoints", "15", "--rays", str(n), "--seed", str(seed), "--outpath", str(tmp_path)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = open(tmp_path / "energy_scan.csv").read().splitlines()
    assert lines[0] == "Energy [keV],efficiency,efficiency error,passed X-rays,effective area [cm^2]" and len(lines) == 16
    got = np.array([[float(x) for x in l.split(",")] for l in lines[1:]])
    full = sa.initFullSetup(flags=L.CF_XRAY_TEST)
    with sa.RayTracer(full) as rt:
        res = sa.performEnergyScan(rt, np.linspace(1, 8, 15), n, seed=seed, flags=L.CF_XRAY_TEST)
    assert np.array_equal(got[:, 0], np.linspace(1, 8, 15))
    np.testing.assert_allclose(got[:, 1], res["efficiency"], rtol=1e-12)
    np.testing.assert_allclose(got[:, 2], res["sigma"] / n, rtol=1e-12)
    assert np.array_equal(got[:, 3], res["n_passed"])
    np.testing.assert_allclose(got[:, 4], res["effective_area_cm2"], rtol=1e-12)
