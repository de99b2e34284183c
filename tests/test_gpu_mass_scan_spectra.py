"""Banded mass scan (include/sart.h: sart_trace_mass_scan_spectra) on the MI355X box: per axion mass and energy band the sum of w and
of w^2 of the fused scan, from one trace of the rays.

The references are launches the project already has, on the same ray ids after sart_set_axion_mass(m_k):
  * sum of w per band   = the band's bins of `energy_weights` of a single-mass spectra launch (it shares q_w with SUM_WEIGHTS:
                          bit for bit in FIXED64);
  * sum of w^2 per band = the origin map's SART_ORIGIN_SUM_WEIGHTS_SQ summed over the radii at the band's indices (exact in FIXED64);
  * the scan rows       = sart_trace_mass_scan_device's, bit for bit.
1e6 rays, 34 masses (two launch groups; zero, the resonance, a far-off point).  Everything one kernel variant needs is computed once
(reference()) and shared by the tests."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import solaraxionraytracing_amd as sa
from solaraxionraytracing_amd import _lib as L

from tests.conftest import make_setup
from tests.test_gpu_mass_scan import VARIANTS, env, masses, variant_setup

pytestmark = pytest.mark.gpu

N, SEED = 1_000_000, 17
N_MASSES = 34
N_IMG = 256 * 256
NR = 16                       # radial bins of the single-mass spectra launches (not looked at)
NAMES = ["gas_pathc", "gas_ring_path", "generic", "generic_rotated", "xray_test_source", "cast_llnl_gas"]
SOLAR = [n for n in NAMES if n != "xray_test_source"]
# Band sets (energy-index space; the small tables have 300 energies, 1e-3 .. 15 keV, index 300 = the X-ray test source):
BANDS = {
    "window31": (20, 3, 31),      # indices 20 .. 112 (1.0 - 5.6 keV): rays below and above it
    "one": (0, 301, 1),           # every passed lane of a wave hits ONE LDS cell per mass and quantity: the worst conflict
    "nothing": (5000, 1, 4),      # every ray in the outside cell
}
_CACHE = {}


def zeros(torch, n, dtype):
    t = torch.zeros(int(n), dtype=dtype, device="cuda")
    torch.cuda.synchronize()      # (the library adds on its own stream)
    return t


def spectra_params(rt, n, seed, off=0, flags=None, accumulate=False):
    p = rt.trace_params(n, seed=seed, ray_id_offset=off, flags=flags, accumulate=accumulate)
    p.spectra, p.n_radial_bins, p.radial_max = 1, NR, 10.0
    return p


def single_spectra(rt, torch, m, n, seed, flags, dtype):
    """(scalars, energy_counts, energy_weights) of one single-mass spectra launch, accumulate = 0; raw slots."""
    ne1 = rt.full.energies.size + 1
    acc = zeros(torch, N_IMG + L.SART_ACC_COUNT + 2 * NR + 3 * ne1, dtype)
    rt.set_axion_mass(float(m))
    rt.trace_histogram_device(spectra_params(rt, n, seed, flags=flags), acc.data_ptr())
    rt.synchronize()
    a = acc.cpu().numpy()
    o = N_IMG + L.SART_ACC_COUNT + 2 * NR
    return a[N_IMG:N_IMG + L.SART_ACC_COUNT].copy(), a[o:o + ne1].copy(), a[o + ne1:o + 2 * ne1].copy()


def origin_sq_per_energy(rt, torch, m, n, seed, flags):
    """Raw FIXED64: sum over the radii of SART_ORIGIN_SUM_WEIGHTS_SQ per energy index, after sart_set_axion_mass(m)."""
    n_e = rt.full.energies.size
    p = rt.origin_params(n, seed, 0, flags, spectra=True, n_radial_bins=NR)
    acc = zeros(torch, N_IMG + L.SART_ACC_COUNT + 2 * NR + 3 * (n_e + 1), torch.int64)
    blk = zeros(torch, rt.origin_block_len(), torch.int64)
    rt.set_axion_mass(float(m))
    rt.trace_origin_device(p, acc.data_ptr(), blk.data_ptr())
    rt.synchronize()
    cells = blk.cpu().numpy()[L.ORIGIN_HEAD:].reshape(-1, n_e, L.ORIGIN_CELL)
    return cells[:, :, L.ORIGIN["SUM_WEIGHTS_SQ"]].sum(axis=0)


def banded(rt, torch, ms, bands, pieces, seed, flags, dtype):
    """Raw scan rows [n + 1][8] and spectra [n + 1][n_bands + 1][4] of the banded scan over `pieces` of ray ids (accumulating calls)."""
    scan = zeros(torch, sa.mass_scan_len(len(ms)), dtype)
    spec = zeros(torch, L.mass_scan_spectra_len(len(ms), bands[2]), dtype)
    for lo, hi in pieces:
        p = rt.trace_params(hi - lo, seed=seed, ray_id_offset=lo, flags=flags, accumulate=True)
        rt.trace_mass_scan_spectra_device(p, ms, bands, scan.data_ptr(), spec.data_ptr())
    rt.synchronize()
    return scan.cpu().numpy().reshape(len(ms) + 1, L.SCAN_ROW), spec.cpu().numpy().reshape(len(ms) + 1, bands[2] + 1, L.MSPEC_CELL)


def plain_scan(rt, torch, ms, n, seed, flags, dtype):
    scan = zeros(torch, sa.mass_scan_len(len(ms)), dtype)
    rt.trace_mass_scan_device(rt.trace_params(n, seed=seed, flags=flags, accumulate=True), ms, scan.data_ptr())
    rt.synchronize()
    return scan.cpu().numpy().reshape(len(ms) + 1, L.SCAN_ROW)


def reference(name):
    """Everything the FIXED64 tests compare for one kernel variant, computed once: the single-mass launches, the plain scan, the banded
    scans of every band set (whole, and the rays split over two accumulating calls), the origin maps (solar source)."""
    if name in _CACHE:
        return _CACHE[name]
    import torch
    full, knobs, flags = variant_setup(name)
    ms = masses(N_MASSES)
    with env(**knobs):
        with sa.RayTracer(full) as rt:
            rt.set_accumulation_mode("fixed64")
            ref = dict(ms=ms, n_e=full.energies.size, test_active=bool(full.setup.test_active))
            ref["banded"] = {k: banded(rt, torch, ms, b, [(0, N)], SEED, flags, torch.int64) for k, b in BANDS.items()}
            ref["split"] = {k: banded(rt, torch, ms, b, [(0, 400_001), (400_001, N)], SEED, flags, torch.int64) for k, b in BANDS.items()}
            ref["plain"] = plain_scan(rt, torch, ms, N, SEED, flags, torch.int64)
            singles = [single_spectra(rt, torch, m, N, SEED, flags, torch.int64) for m in ms]
            ref["scalars"] = np.array([s[0] for s in singles])
            ref["energy_counts"] = np.array([s[1] for s in singles])
            ref["energy_weights"] = np.array([s[2] for s in singles])
            # the rays on the detector whose mass-independent weight factor is non-zero: the passed rays of a launch that leaves the
            # conversion probability out of the weight
            no_prob = (full.flags if flags is None else flags) | L.CF_IGNORE_CONV_PROB
            ref["on_detector"] = single_spectra(rt, torch, ms[1], N, SEED, no_prob, torch.int64)[1]
            if not ref["test_active"]:
                ref["origin_sq"] = np.array([origin_sq_per_energy(rt, torch, m, N, SEED, flags) for m in ms])
    _CACHE[name] = ref
    return ref


def limbs(cells, key):
    """hi 2^40 + lo of a raw two-limb sum, as Python integers (object array)."""
    lo, hi = cells[..., L.MSPEC[key]].astype(object), cells[..., L.MSPEC_HI[key]].astype(object)
    return hi * (1 << L.FIXED_LIMB_BITS) + lo


def row_limbs(rows, key):
    return rows[..., L.SCAN_HI[key]].astype(object) * (1 << L.FIXED_LIMB_BITS) + rows[..., L.SCAN[key]].astype(object)


def band_sums(per_index, bands):
    """[..., n_e1] per energy index -> [..., n_bands + 1] per cell, as Python integers / floats, binned with the CPU-pinned helper."""
    cell = sa.band_of_energy_index(np.arange(per_index.shape[-1]), bands)
    out = np.zeros(per_index.shape[:-1] + (bands[2] + 1,), dtype=object if per_index.dtype.kind == "i" else np.float64)
    for c in range(bands[2] + 1):
        out[..., c] = per_index[..., cell == c].astype(out.dtype).sum(axis=-1)
    return out


# ---- 1: FIXED64, bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fixed64_cells_equal_the_band_sums_of_single_mass_spectra_bit_for_bit(name):
    assert set(NAMES) <= set(VARIANTS)
    ref = reference(name)
    n_m = N_MASSES
    k_res = 1                                               # masses()[1] is the resonance
    counts_res = ref["energy_counts"][k_res]
    if ref["test_active"]:
        assert counts_res[:-1].sum() == 0 and counts_res[-1] > 1000          # every ray has index n_energies
    else:
        # the bands used for the comparison hold rays: each of the 31, and both sides of the window, in the single launch alone
        per_cell = band_sums(counts_res, BANDS["window31"])
        assert per_cell.min() > 0, per_cell
        assert counts_res[:20].sum() > 0 and counts_res[113:].sum() > 0
    for key, bands in BANDS.items():
        rows, cells = ref["banded"][key]
        # the scan rows are those of the plain scan, the rays split over two calls give the same bits
        assert np.array_equal(rows, ref["plain"]), (name, key)
        assert np.array_equal(rows, ref["split"][key][0]) and np.array_equal(cells, ref["split"][key][1]), (name, key)
        # every cell's sum of w = the band's bins of the single-mass launch
        want = band_sums(ref["energy_weights"], bands)
        got = limbs(cells[:n_m], "SUM_WEIGHTS")
        assert np.array_equal(got, want), (name, key, np.argwhere(got != want)[:5])
        assert (cells[:n_m, :, L.MSPEC["SUM_WEIGHTS"]] < 2 ** L.FIXED_LIMB_BITS).all() and (cells >= 0).all()
        # conservation: the cells of a mass add up to its row, the counts to N_ON_DETECTOR
        for q in ("SUM_WEIGHTS", "SUM_WEIGHTS_SQ"):
            assert np.array_equal(limbs(cells[:n_m], q).sum(axis=1), row_limbs(rows[:n_m], q)), (name, key, q)
        counts = cells[n_m, :, L.MSPEC_COUNTS["N_ON_DETECTOR"]]
        assert counts.sum() == rows[n_m, L.SCAN_SHARED["N_ON_DETECTOR"]] > 1000
        assert not cells[n_m, :, 1:].any()
        # per band: the passed rays of the launch without the conversion probability (a few rays' probability is exactly zero even on
        # the resonance, so a single-mass launch counts no more than that)
        assert np.array_equal(counts.astype(object), band_sums(ref["on_detector"], bands)), (name, key)
        assert (counts.astype(object) >= band_sums(counts_res, bands)).all() and rows[k_res, L.SCAN["N_PASSED"]] == counts_res.sum()
        if key == "nothing":
            assert not cells[:, :bands[2]].any()
        if key == "one":
            assert not cells[:, 1].any()       # the window covers every index: nothing outside
    # the single launches themselves agree with the scan rows (what test_gpu_mass_scan holds; here: the spectra launch is the same launch)
    assert np.array_equal(ref["scalars"][:, L.ACC["SUM_WEIGHTS"]], ref["plain"][:n_m, L.SCAN["SUM_WEIGHTS"]])


# ---- 2: sum of w^2 per band ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SOLAR)
def test_fixed64_squared_weights_per_band_equal_the_origin_map(name):
    ref = reference(name)
    sq = np.concatenate([ref["origin_sq"], np.zeros((N_MASSES, 1), dtype=np.int64)], axis=1)      # (index n_energies: the test source only)
    assert sq[1].sum() > 0
    for key, bands in BANDS.items():
        cells = ref["banded"][key][1]
        got, want = limbs(cells[:N_MASSES], "SUM_WEIGHTS_SQ"), band_sums(sq, bands)
        assert np.array_equal(got, want), (name, key, np.argwhere(got != want)[:5])


# ---- 3: f64 mode ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gas_pathc", "gas_ring_path", "generic_rotated"])
def test_f64_cells_equal_single_mass_spectra(name):
    """test_f64_scan_equals_single_mass_launches' tolerances (1e-12 on the flux, 1e-11 on the squares: summation order), per band."""
    import torch
    full, knobs, flags = variant_setup(name)
    ms = masses(N_MASSES)
    bands = BANDS["window31"]
    with env(**knobs):
        with sa.RayTracer(full) as rt:
            rows, cells = banded(rt, torch, ms, bands, [(0, N)], SEED, flags, torch.float64)
            plain = plain_scan(rt, torch, ms, N, SEED, flags, torch.float64)
            per_mass, shared, spec = rt.trace_mass_scan_spectra(ms, bands, N, seed=SEED, flags=flags)      # the blocking form
            singles = [single_spectra(rt, torch, m, N, SEED, flags, torch.float64) for m in ms]
            on_det = single_spectra(rt, torch, ms[1], N, SEED, (full.flags if flags is None else flags) | L.CF_IGNORE_CONV_PROB, torch.float64)[1]
    ew = np.array([s[2] for s in singles])
    want = band_sums(ew, bands)
    assert want[1].min() > 0
    got = cells[:N_MASSES, :, L.MSPEC["SUM_WEIGHTS"]]
    assert np.abs(got / want - 1.0).max() < 1e-12
    assert np.abs(spec["SUM_WEIGHTS"] / want - 1.0).max() < 1e-12
    assert not cells[:, :, L.MSPEC_HI["SUM_WEIGHTS"]].any() and not cells[:, :, L.MSPEC_HI["SUM_WEIGHTS_SQ"]].any()
    for q, tol in (("SUM_WEIGHTS", 1e-12), ("SUM_WEIGHTS_SQ", 1e-11)):
        assert np.abs(rows[:N_MASSES, L.SCAN[q]] / plain[:N_MASSES, L.SCAN[q]] - 1.0).max() < tol
        assert np.abs(cells[:N_MASSES, :, L.MSPEC[q]].sum(axis=1) / rows[:N_MASSES, L.SCAN[q]] - 1.0).max() < tol
        assert per_mass[q] == pytest.approx(rows[:N_MASSES, L.SCAN[q]], rel=tol)
    for k, s in enumerate(singles):
        assert rows[k, L.SCAN["SUM_WEIGHTS_SQ"]] == pytest.approx(s[0][L.ACC["SUM_WEIGHTS_SQ"]], rel=1e-11)
    assert np.array_equal(rows[:, L.SCAN["N_PASSED"]], plain[:, L.SCAN["N_PASSED"]]) and np.array_equal(rows[N_MASSES], plain[N_MASSES])
    counts = cells[N_MASSES, :, L.MSPEC_COUNTS["N_ON_DETECTOR"]]
    assert np.array_equal(counts, band_sums(on_det, bands)) and np.array_equal(spec["N_ON_DETECTOR"], counts)


# ---- 4: against the CPU oracle, per mass and band --------------------------------------------------------------------------------------
@pytest.mark.parametrize("tables", ["small", "small_xray"])
def test_cells_match_the_oracle_per_mass_and_band(tables):
    """test_scan_matches_the_oracle_per_mass' setups, rays and masses (small tables, 1e5 rays, nine masses: the 80-bit oracle takes
    its time), its envelope for the flux (1e-6; a band's counts are held exactly, so the rays are the same), per band: the oracle's
    passed records binned with band_of_energy_index."""
    from oracle.oracle import Oracle
    full = variant_setup("xray_test_source")[0] if tables == "small_xray" else make_setup("babyiaxo_xmm_gas")
    ms = masses(9)
    n, seed = 100_000, 4
    bands = (0, 301, 1) if tables == "small_xray" else (20, 6, 15)       # indices 20 .. 109 in 15 bands
    with sa.RayTracer(full) as rt:
        per_mass, shared, spec = rt.trace_mass_scan_spectra(ms, bands, n, seed=seed)
    o = Oracle(full, "ld")
    ne = full.energies.size

    def binned(rec):
        passed = rec[rec["passed"] != 0]
        e_idx = np.full(passed.size, ne) if full.setup.test_active else np.searchsorted(full.energies, passed["energiesAx"])
        cell = sa.band_of_energy_index(e_idx, bands)
        return passed.size, np.bincount(cell, minlength=bands[2] + 1), np.bincount(cell, weights=passed["weights"], minlength=bands[2] + 1)

    # the counts: the oracle's passed rays without the conversion probability in the weight (N_ON_DETECTOR's definition)
    want_n = binned(o.trace_records(n, seed=seed, flags=full.flags | L.CF_IGNORE_CONV_PROB))[1]
    assert np.array_equal(spec["N_ON_DETECTOR"], want_n), (spec["N_ON_DETECTOR"], want_n)
    assert want_n.sum() == shared["N_ON_DETECTOR"] > 1000 and (tables == "small_xray" or want_n.min() > 0)
    for k, m in enumerate(ms):
        s = full.setup.copy()
        s.m_axion = float(m)
        n_passed, _, want_w = binned(o.trace_records(n, seed=seed, setup=s))
        assert per_mass["N_PASSED"][k] == n_passed
        filled = want_w > 0
        assert np.array_equal(spec["SUM_WEIGHTS"][k] > 0, filled)
        assert np.abs(spec["SUM_WEIGHTS"][k][filled] / want_w[filled] - 1.0).max() < 1e-6, (k, m)
        assert spec["SUM_WEIGHTS"][k].sum() == pytest.approx(per_mass["SUM_WEIGHTS"][k], rel=1e-12)


# ---- 5: finalize and flags ------------------------------------------------------------------------------------------------------------
def test_fixed64_finalize_equals_finalized_single_launches():
    """The quanta of mass k are those of a single launch with that mass: a finalized cell is the correctly rounded sum of the band's
    finalized energy_weights bins (both are exact multiples of the quantum, rounded once), bit for bit; the blocking call returns it."""
    full = make_setup("babyiaxo_xmm_gas")
    ms = masses(7)
    bands = BANDS["window31"]
    n, seed = 1_000_000, 3
    cell_of = sa.band_of_energy_index(np.arange(full.energies.size + 1), bands)
    with sa.RayTracer(full) as rt:
        rt.set_accumulation_mode("fixed64")
        per_mass, shared, spec = rt.trace_mass_scan_spectra(ms, bands, n, seed=seed)
        plain, plain_shared = rt.trace_mass_scan(ms, n, seed=seed)
        for k, m in enumerate(ms):
            rt.set_axion_mass(float(m))
            _, s, sp = rt.trace_spectra(n, seed=seed, n_radial_bins=NR)
            for c in range(bands[2] + 1):
                want = math.fsum(sp["energy_weights"][cell_of == c])
                assert np.float64(spec["SUM_WEIGHTS"][k, c]).view(np.uint64) == np.float64(want).view(np.uint64), (k, c, spec["SUM_WEIGHTS"][k, c], want)
            for key in ("SUM_WEIGHTS", "SUM_WEIGHTS_SQ", "N_PASSED"):
                assert np.float64(per_mass[key][k]).view(np.uint64) == np.float64(s[key]).view(np.uint64) == np.float64(plain[key][k]).view(np.uint64)
    assert shared == plain_shared and spec["N_ON_DETECTOR"].sum() == shared["N_ON_DETECTOR"]
    assert np.all(np.isfinite(spec["SUM_WEIGHTS_SQ"])) and spec["SUM_WEIGHTS_SQ"][:, :-1].min() > 0
    assert spec["SUM_WEIGHTS_SQ"].sum(axis=1) == pytest.approx(per_mass["SUM_WEIGHTS_SQ"], rel=1e-12)


@pytest.mark.parametrize("flags", [L.CF_IGNORE_DET_WINDOW | L.CF_IGNORE_GAS_ABS, L.CF_IGNORE_REFLECTION,
                                   L.CF_IGNORE_DET_WINDOW | L.CF_IGNORE_REFLECTION | L.CF_IGNORE_GAS_ABS])
def test_fixed64_cells_equal_single_mass_spectra_under_the_ignore_flags(flags):
    import torch
    full = make_setup("babyiaxo_xmm_gas")
    ms = masses(6)
    bands = BANDS["window31"]
    with sa.RayTracer(full) as rt:
        rt.set_accumulation_mode("fixed64")
        rows, cells = banded(rt, torch, ms, bands, [(0, N)], 23, flags, torch.int64)
        plain = plain_scan(rt, torch, ms, N, 23, flags, torch.int64)
        ew = np.array([single_spectra(rt, torch, m, N, 23, flags, torch.int64)[2] for m in ms])
        # the finalize accepts what the launch wrote
        out = zeros(torch, rows.size + cells.size, torch.float64)
        d_rows, d_cells = torch.from_numpy(rows.ravel()).cuda(), torch.from_numpy(cells.ravel()).cuda()
        torch.cuda.synchronize()
        rt.finalize_mass_scan_spectra_device(rt.trace_params(N, seed=23, flags=flags), ms, bands, d_rows.data_ptr(), d_cells.data_ptr(), out.data_ptr())
        rt.synchronize()
    assert np.array_equal(rows, plain)
    assert np.array_equal(limbs(cells[:len(ms)], "SUM_WEIGHTS"), band_sums(ew, bands)) and ew[1].sum() > 0
    fin = out.cpu().numpy()[rows.size:].reshape(cells.shape)
    assert np.all(fin[:len(ms), :, L.MSPEC["SUM_WEIGHTS"]].sum(axis=1) > 0) and not fin[:, :, 2:].any()


def _setup_bytes(rt):
    s = L.Setup()
    L.check(rt.lib.sart_get_setup(rt.handle, C.byref(s)))
    return bytes(s)


def test_refused_calls_leave_the_context_unchanged():
    import torch
    ms = masses(5)
    vac = make_setup("babyiaxo_xmm")
    with sa.RayTracer(vac) as rt:
        before = _setup_bytes(rt)
        with pytest.raises(L.SartError) as e:
            rt.trace_mass_scan_spectra(ms, (0, 10, 8), 1000)
        assert e.value.code == L.SART_ERR_INVALID_ARGUMENT and "vacuum" in str(e.value)
        assert _setup_bytes(rt) == before
    full = make_setup("babyiaxo_xmm_gas")
    with sa.RayTracer(full) as rt:
        before = _setup_bytes(rt)
        want = rt.trace_mass_scan(ms, 50_000, seed=2)[0]["SUM_WEIGHTS"]
        for bad in ((0, 10, 0), (0, 10, 32), (0, 0, 8), (0, -3, 8), (-1, 10, 8)):
            with pytest.raises(L.SartError) as e:
                rt.trace_mass_scan_spectra(ms, bad, 1000)
            assert e.value.code == L.SART_ERR_INVALID_ARGUMENT, bad
            assert _setup_bytes(rt) == before
        scan = zeros(torch, sa.mass_scan_len(len(ms)), torch.float64)
        spec = zeros(torch, L.mass_scan_spectra_len(len(ms), 8), torch.float64)
        p = rt.trace_params(1000, seed=2)
        b = L.EnergyBands(0, 10, 8)
        m = np.ascontiguousarray(ms)
        for args in ((C.byref(b), C.c_void_p(scan.data_ptr()), None), (C.byref(b), None, C.c_void_p(spec.data_ptr())),
                     (None, C.c_void_p(scan.data_ptr()), C.c_void_p(spec.data_ptr()))):
            assert rt.lib.sart_trace_mass_scan_spectra_device(rt.handle, C.byref(p), L.as_dp(m), len(ms), *args) == L.SART_ERR_INVALID_ARGUMENT
        assert rt.lib.sart_trace_mass_scan_spectra_device(rt.handle, C.byref(p), None, len(ms), C.byref(b), C.c_void_p(scan.data_ptr()),
                                                          C.c_void_p(spec.data_ptr())) == L.SART_ERR_INVALID_ARGUMENT
        rt.synchronize()
        assert not scan.cpu().numpy().any() and not spec.cpu().numpy().any()
        assert _setup_bytes(rt) == before
        # and the context still computes what it computed (f64: up to the summation order)
        assert rt.trace_mass_scan(ms, 50_000, seed=2)[0]["SUM_WEIGHTS"] == pytest.approx(want, rel=1e-12)
        per_mass, _, sp = rt.trace_mass_scan_spectra(ms, (0, 10, 8), 50_000, seed=2)
        assert per_mass["SUM_WEIGHTS"] == pytest.approx(want, rel=1e-12) and sp["SUM_WEIGHTS"].sum(axis=1) == pytest.approx(want, rel=1e-12)
        # no rays: zeros
        per_mass, sh, sp = rt.trace_mass_scan_spectra(ms, (0, 10, 8), 0, seed=2)
        assert not per_mass["SUM_WEIGHTS"].any() and not sp["SUM_WEIGHTS"].any() and sh["N_RAYS"] == 0


@pytest.mark.parametrize("craft", ["stray_quantum", "stray_square", "stray_count", "slot_at_2_62", "clean"])
def test_finalize_reports_a_crafted_raw_buffer(craft):
    """One stray quantum in a cell breaks the conservation law of its mass; a slot at 2^62 is a wrapped slot: SART_ERR_ACCUMULATOR from
    the next synchronize.  The buffers as the launch wrote them pass."""
    import torch
    full = make_setup("babyiaxo_xmm_gas")
    ms = masses(34)
    bands = (20, 6, 15)
    n, seed = 300_000, 5
    with sa.RayTracer(full) as rt:
        rt.set_accumulation_mode("fixed64")
        rows, cells = banded(rt, torch, ms, bands, [(0, n)], seed, None, torch.int64)
        cells = cells.copy()
        if craft == "stray_quantum":
            cells[33, 4, L.MSPEC["SUM_WEIGHTS"]] += 1          # (a mass of the second launch group)
        elif craft == "stray_square":
            cells[2, 15, L.MSPEC["SUM_WEIGHTS_SQ"]] += 1       # (the outside cell)
        elif craft == "stray_count":
            cells[34, 7, L.MSPEC_COUNTS["N_ON_DETECTOR"]] += 1
        elif craft == "slot_at_2_62":
            cells[5, 3, L.MSPEC_HI["SUM_WEIGHTS_SQ"]] = 1 << 62
        d_rows, d_cells = torch.from_numpy(rows.ravel().copy()).cuda(), torch.from_numpy(cells.ravel()).cuda()
        out = zeros(torch, rows.size + cells.size, torch.float64)
        p = rt.trace_params(n, seed=seed)
        rt.finalize_mass_scan_spectra_device(p, ms, bands, d_rows.data_ptr(), d_cells.data_ptr(), out.data_ptr())
        if craft == "clean":
            rt.synchronize()
            fin = out.cpu().numpy()
            per_mass, shared = sa.split_mass_scan(fin[:rows.size], len(ms))
            spec = sa.split_mass_scan_spectra(fin[rows.size:], len(ms), bands[2])
            assert spec["SUM_WEIGHTS"].sum(axis=1) == pytest.approx(per_mass["SUM_WEIGHTS"], rel=1e-12)
            assert spec["N_ON_DETECTOR"].sum() == shared["N_ON_DETECTOR"] and np.all(np.isfinite(spec["SUM_WEIGHTS_SQ"]))
        else:
            with pytest.raises(L.SartError) as e:
                rt.synchronize()
            assert e.value.code == L.SART_ERR_ACCUMULATOR
            rt.synchronize()                                   # reported once
        # the output needs an array of its own
        with pytest.raises(L.SartError) as e:
            rt.finalize_mass_scan_spectra_device(p, ms, bands, d_rows.data_ptr(), d_cells.data_ptr(), d_cells.data_ptr())
        assert e.value.code == L.SART_ERR_INVALID_ARGUMENT


# ---- 6: the command line, end to end -----------------------------------------------------------------------------------------------------
def test_cli_rows_add_up_to_the_mass_scan_csv(tmp_path):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sample = open(os.path.join(root, "tools", "make_nim_parity_kit.py")).read()
    cfg = tmp_path / "config.toml"
    cfg.write_text(sample.split('CONFIG_TEMPLATE = """')[1].split('"""')[0] % ("BabyIAXO", "InGridIAXO", "gas", "XMM"))
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, "-m", "solaraxionraytracing_amd", "--rays", "300000", "--outpath", str(out), "--config", str(cfg),
                        "--massScanMin", "0.004", "--massScanMax", "0.012", "--numMassScanPoints", "9", "--massScanBands", "12"],
                       capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    ms = np.loadtxt(out / "axion_mass_scan.csv", delimiter=",", skiprows=1)
    sp = np.loadtxt(out / "axion_mass_scan_spectra.csv", delimiter=",", skiprows=1)
    assert ms.shape == (9, 5) and sp.shape == (9 * 13, 7) and int(np.argmax(ms[:, 1])) == 4
    sp = sp.reshape(9, 13, 7)
    assert np.array_equal(sp[:, 0, 0], ms[:, 0]) and np.array_equal(sp[0, :, 1], np.arange(13))
    assert sp[:, :, 4].sum(axis=1) == pytest.approx(ms[:, 1], rel=1e-12)
    assert np.sqrt((sp[:, :, 5] ** 2).sum(axis=1)) == pytest.approx(ms[:, 2], rel=1e-9)
    assert np.all(np.isnan(sp[:, 12, 2:4])) and np.all(np.diff(sp[0, :12, 2]) > 0) and np.allclose(sp[0, 1:12, 2], sp[0, :11, 3])
    assert sp[0, :, 6].sum() >= ms[:, 3].max() and np.array_equal(sp[0, :, 6], sp[8, :, 6])
    # the band where the signal peaks moves with the mass only through its shape: every mass has its flux inside the bands
    assert np.all(sp[:, :12, 4].sum(axis=1) > 0.9 * ms[:, 1])
    assert "wrote" in r.stdout and "axion_mass_scan_spectra.csv" in r.stdout
