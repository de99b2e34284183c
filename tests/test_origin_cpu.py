"""CPU side of the solar-origin map (include/sart.h: sart_trace_histogram_origin_device): the C-ABI tables, the Nim binding, the code
object of origin_histogram_kernel, origin.py on hand-made maps, the command line's new switch, the reweight module on a saved map,
and the reweighting identity itself on the CPU oracle alone: a map built from one oracle trace, reweighted to another emission
table, against an independent oracle trace of that table.

Measured pull of the identity (fixed seeds, 1e5 rays each, SMALL Primakoff table, g in [0.5, 2]): see
test_reweighting_identity_on_the_oracle."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import solaraxionraytracing_amd as sa
from solaraxionraytracing_amd import _lib as L
from solaraxionraytracing_amd import origin, reweight, tables
from solaraxionraytracing_amd import raytracer as R
from solaraxionraytracing_amd.__main__ import build_parser, check_scan_args

from tests.conftest import SMALL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
NEW = ("sart_origin_block_len", "sart_trace_histogram_origin_device", "sart_trace_histogram_origin", "sart_finalize_origin_device")


def test_entry_points_are_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sart.h")).read(), flags=re.S)
    nim = open(os.path.join(ROOT, "integration", "sart_ffi.nim")).read()
    lib = L.load_sart()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in L.SART_SYMBOLS, name
        assert re.search(r"proc %s\*" % name, nim), name
        assert hasattr(lib, name), name
    assert lib.sart_abi_version() == 5
    assert C.sizeof(L.TraceParams) == 88


def test_layout_constants_agree_across_header_library_and_python():
    hdr = open(os.path.join(ROOT, "include", "sart.h")).read()
    for key, slot in L.ORIGIN.items():
        assert re.search(r"SART_ORIGIN_%s = %d\b" % (key, slot), hdr), key
    assert re.search(r"SART_ORIGIN_N_PASSED = %d\b" % L.ORIGIN_HEAD_SLOTS["N_PASSED"], hdr)
    for key, slot in L.ORIGIN_HEAD_HI.items():
        assert re.search(r"SART_ORIGIN_%s_HI = %d\b" % (key, slot), hdr), key
    assert re.search(r"SART_ORIGIN_CELL = %d\b" % L.ORIGIN_CELL, hdr) and re.search(r"SART_ORIGIN_HEAD = %d\b" % L.ORIGIN_HEAD, hdr)
    assert L.ORIGIN_CELL == 4 and L.ORIGIN_HEAD == 8     # one aligned 32-byte cell per (r, e)
    lib = L.load_sart()
    for nr, ne in ((400, 300), (1968, 1500), (1, 1), (8, 16), (0, 5), (-3, 5)):
        want = 8 + max(nr, 0) * max(ne, 0) * 4
        assert lib.sart_origin_block_len(nr, ne) == L.origin_block_len(nr, ne) == R.origin_block_len(nr, ne) == want


def test_origin_kernel_instantiations_meet_the_ray_kernel_budgets(tmp_path):
    """Exactly {not rotated, rotated} x {f64, FIXED64}, named without `trace_`; no scratch, no spills, <= 128 VGPRs, and the LDS of
    the sibling breakdown kernels."""
    obj = tmp_path / "sart_kernels.o"
    shutil.copy(os.path.join(ROOT, "solaraxionraytracing_amd", "csrc", "build", "sart_kernels.o"), obj)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", str(obj)], check=True, capture_output=True, cwd=tmp_path)
    dev = [f for f in os.listdir(tmp_path) if "amdgcn" in f]
    assert len(dev) == 1, dev
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(tmp_path / dev[0])], capture_output=True, text=True,
                           check=True).stdout
    found, lds = {}, {}
    for k in re.split(r"\n  - \.a", notes):
        m = re.search(r"\.name:\s+(\S+)", k)
        if not m:
            continue
        g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, k).group(1))
        if "origin_histogram_kernel" in m.group(1):
            found[m.group(1)] = (g("private_segment_fixed_size"), g("vgpr_spill_count"), g("vgpr_count"), g("group_segment_fixed_size"))
        elif "channel_histogram_kernel" in m.group(1) or "shell_histogram_kernel" in m.group(1):
            lds[m.group(1)] = g("group_segment_fixed_size")
    want = {"_ZN4sart23origin_histogram_kernelILi1024ELb%dELb%dEEEvNS_4HotAEPKNS_7DevBlobENS_9TraceArgsEPdNS_4HotBENS_10OriginArgsE" % (r, f)
            for r in (0, 1) for f in (0, 1)}
    assert set(found) == want
    assert len(lds) == 8 and len(set(lds.values())) == 1
    for name, (scratch, spills, vgprs, group) in found.items():
        assert "trace_" not in name
        assert scratch == 0 and spills == 0, name
        assert vgprs <= 128, (name, vgprs)
        assert group == next(iter(lds.values())) <= 160 * 1024, (name, group)


# ---- origin.py on hand-made maps ---------------------------------------------------------------
def hand_map():
    d = np.array([[1.0, 2.0, 0.0], [4.0, 0.0, 8.0]])
    return dict(counts=np.array([[1, 2, 0], [2, 0, 4]]), weights=d, weights_sq=np.array([[1.0, 2.0, 0.0], [8.0, 0.0, 16.0]]),
                radii=np.array([0.1, 0.2]), energies=np.array([1.0, 2.0, 3.0]))


def test_split_origin_names_the_slots():
    blk = np.arange(8 + 2 * 3 * 4, dtype=np.float64)
    o = L.split_origin(blk, 2, 3)
    assert o["head"] == dict(N_PASSED=0.0, SUM_WEIGHTS=1.0, SUM_WEIGHTS_SQ=2.0)
    np.testing.assert_array_equal(o["counts"], [[8, 12, 16], [20, 24, 28]])
    np.testing.assert_array_equal(o["weights"], o["counts"] + 1)
    np.testing.assert_array_equal(o["weights_sq"], o["counts"] + 2)
    with pytest.raises(AssertionError):
        L.split_origin(blk, 3, 2 + 1)


def test_radial_profile_and_acceptance_by_hand():
    m = hand_map()
    np.testing.assert_array_equal(origin.radial_profile(m), [3.0, 12.0])
    rcdf = np.array([0.25, 1.0])
    ecdf = np.array([[0.5, 1.0, 1.0], [0.2, 0.2, 1.0]])
    mass = origin.cell_mass(rcdf, ecdf)
    np.testing.assert_allclose(mass, [[0.125, 0.125, 0.0], [0.15, 0.0, 0.6]], rtol=1e-15, atol=1e-17)
    assert mass.sum() == pytest.approx(1.0, rel=1e-15)
    a = origin.acceptance(m, rcdf, ecdf, 100)
    np.testing.assert_allclose(a[[0, 0, 1, 1], [0, 1, 0, 2]], [1 / 12.5, 2 / 12.5, 4 / 15.0, 8 / 60.0], rtol=1e-14)
    assert np.isnan(a[0, 2]) and np.isnan(a[1, 1])
    with pytest.raises(ValueError):
        origin.acceptance(m, rcdf, ecdf.T, 100)


def test_reweight_by_hand():
    m = hand_map()
    old = np.array([[1.0, 2.0, 4.0], [2.0, 0.0, 4.0]])
    new = np.array([[2.0, 1.0, 4.0], [2.0, 0.0, 1.0]])
    r = origin.reweight(m, old, new)
    # rho = [[2, 1/2, 1], [1, -, 1/4]]
    assert r["flux"] == 2.0 + 1.0 + 0.0 + 4.0 + 2.0
    assert r["flux_error"] == pytest.approx(np.sqrt(1.0 * 4 + 2.0 / 4 + 8.0 + 16.0 / 16), rel=1e-15)
    np.testing.assert_array_equal(r["spectrum"], [6.0, 1.0, 2.0])
    np.testing.assert_array_equal(r["radial_profile"], [3.0, 6.0])
    assert r["uncovered"] == 0.0 and r["rho"][1, 1] == 0.0
    same = origin.reweight(m, old, old)
    assert same["flux"] == m["weights"].sum() and same["flux_error"] == np.sqrt(m["weights_sq"].sum())
    np.testing.assert_array_equal(same["radial_profile"], origin.radial_profile(m))
    # planted errors: a transposed map is refused, a ratio taken the wrong way round gives another number
    with pytest.raises(ValueError):
        origin.reweight(dict(m, weights=m["weights"].T, weights_sq=m["weights_sq"].T), old, new)
    assert origin.reweight(m, new, old)["flux"] != r["flux"]
    assert origin.reweight(m, new, old)["flux"] == 0.5 + 4.0 + 4.0 + 32.0
    with pytest.raises(ValueError):
        origin.reweight(m, old, -new)


def test_reweight_uncovered_cap_from_both_sides():
    m = hand_map()
    old = np.array([[1.0, 2.0, 4.0], [2.0, 0.0, 4.0]])
    new = old.copy()
    new[1, 1] = 3.0                                   # mass where nothing was sampled: 3 x 2^2 x 0.2^2 = 0.48
    mass = origin.model_mass(new, m["radii"], m["energies"])
    share = 0.48 / mass.sum()
    assert mass[1, 1] == pytest.approx(0.48, rel=1e-15)
    with pytest.raises(origin.UncoveredError):
        origin.reweight(m, old, new)                  # the default cap is 0
    with pytest.raises(origin.UncoveredError):
        origin.reweight(m, old, new, max_uncovered=share * (1 - 1e-9))
    r = origin.reweight(m, old, new, max_uncovered=share * (1 + 1e-9))
    assert r["uncovered"] == pytest.approx(share, rel=1e-14) and r["flux"] == m["weights"].sum()
    assert np.all(np.isfinite(r["rho"])) and r["rho"][1, 1] == 0.0            # no ratio where rates_old == 0
    # without a grid the share cannot be told
    bare = {k: m[k] for k in ("counts", "weights", "weights_sq")}
    with pytest.raises(ValueError):
        origin.reweight(bare, old, new, max_uncovered=1.0)
    assert origin.reweight(bare, old, new, max_uncovered=1.0, radii=m["radii"], energies=m["energies"])["uncovered"] == r["uncovered"]
    # weight in a cell the "old" rates cannot have sampled: these are not the map's rates
    wrong = old.copy()
    wrong[0, 0] = 0.0
    with pytest.raises(ValueError):
        origin.reweight(m, wrong, new, max_uncovered=1.0)


# ---- the command line --------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [["--xrayTest"], ["--shellBreakdown"], ["--emissionChannels", "terms"], ["--massScanMin", "0", "--massScanMax", "0.1"],
                                   ["--angularScanMin", "0", "--angularScanMax", "0.1"], ["--energyScanMin", "1", "--energyScanMax", "2"]])
def test_cli_refuses_origin_map_beside_other_modes(extra):
    ap = build_parser()
    args = ap.parse_args(["--originMap"] + extra)
    with pytest.raises(SystemExit) as e:
        check_scan_args(ap, args)
    assert e.value.code == 2
    check_scan_args(ap, ap.parse_args(["--originMap"]))      # alone it is fine
    assert ap.parse_args([]).originMap is False


def test_reweight_module_on_a_saved_map(tmp_path, capsys):
    m = hand_map()
    old = np.array([[1.0, 2.0, 4.0], [2.0, 0.0, 4.0]])
    path = str(tmp_path / "origin_map_IAXO.npz")
    np.savez_compressed(path, counts=m["counts"], weights=m["weights"], weights_sq=m["weights_sq"], radii=m["radii"],
                        energies=m["energies"], n_rays=np.float64(1000), rates=old)
    new = np.array([[2.0, 1.0, 4.0], [2.0, 0.0, 1.0]])
    csv = str(tmp_path / "model.csv")
    tables.write_solar_model_csv(csv, m["radii"], m["energies"], new)
    assert reweight.main([path, "--solarModel", csv]) == 0
    out = capsys.readouterr().out
    assert "reweighted flux 9 +- " in out and "uncovered 0" in out and "traced flux 15 +- " in out
    s_old, s_new = origin.model_mass(old, m["radii"], m["energies"]).sum(), origin.model_mass(new, m["radii"], m["energies"]).sum()
    direct = float([l for l in out.splitlines() if l.startswith("as a direct trace")][0].split()[-3])
    assert direct == pytest.approx(9.0 * s_old / s_new, rel=1e-15)
    new[1, 1] = 3.0
    tables.write_solar_model_csv(csv, m["radii"], m["energies"], new)
    assert reweight.main([path, "--solarModel", csv]) == 1
    assert "never sampled" in capsys.readouterr().err
    assert reweight.main([path, "--solarModel", csv, "--maxUncovered", "0.5"]) == 0
    capsys.readouterr()
    tables.write_solar_model_csv(csv, m["radii"] * 2, m["energies"], new)      # another grid
    with pytest.raises(SystemExit) as e:
        reweight.main([path, "--solarModel", csv])
    assert e.value.code == 2


# ---- the identity itself, on the reference's algorithm alone ------------------------------------
def oracle_map(full, n, seed):
    """The origin map of an oracle trace, cells as tests/test_gpu_channels.py::passed_rays finds them, and the run's flux."""
    from oracle import oracle as O
    rec = O.Oracle(full).trace_records(n, seed=seed)
    ids = np.nonzero(rec["passed"] != 0)[0]
    lib = O.load()
    u = (C.c_double * 6)()
    u2 = np.empty(ids.size)
    for i, rid in enumerate(ids):
        lib.sart_oracle_uniforms(seed, int(rid), u)
        u2[i] = u[2]
    rcdf = full.fluxRadiusCDF
    r_idx = np.minimum(np.searchsorted(rcdf, u2, side="left"), rcdf.size - 1)
    e = rec["energiesAx"][ids]
    e_idx = np.searchsorted(full.energies, e)
    assert np.all(full.energies[e_idx] == e)
    w = rec["weights"][ids]
    shape = (rcdf.size, full.energies.size)
    m = dict(counts=np.zeros(shape, dtype=np.int64), weights=np.zeros(shape), weights_sq=np.zeros(shape))
    np.add.at(m["counts"], (r_idx, e_idx), 1)
    np.add.at(m["weights"], (r_idx, e_idx), w)
    np.add.at(m["weights_sq"], (r_idx, e_idx), w * w)
    return m, float(w.sum()), float((w * w).sum())


def test_reweighting_identity_on_the_oracle():
    """One oracle trace of the SMALL Primakoff table, reweighted to rates' = rates g(r, e), against an independent oracle trace of the
    tables made from rates' (scaled by S'/S: a direct run is normalised to its own table).  Within 5 sigma, sigma^2 = sum (w rho)^2
    of the first run + sum w^2 of the second, scaled likewise.  Measured with these seeds: pull +0.54 sigma (reweighted 4.5985e-5,
    direct scaled 4.5708e-5, sigma 5.12e-7), while the unreweighted flux of the first run lies 16 sigma away."""
    n = 100_000
    full = sa.initFullSetup(**SMALL)
    rates = full.em_rates
    np.testing.assert_array_equal(rates, tables.primakoff_emission_table(SMALL["n_radii"], SMALL["n_energies"]))
    x_r = np.linspace(0.0, 1.0, rates.shape[0])[:, None]
    x_e = np.linspace(0.0, 1.0, rates.shape[1])[None, :]
    g = 0.5 + 0.75 * (1.0 + np.sin(4.0 * x_r + 3.0 * x_e))
    assert g.min() >= 0.5 and g.max() <= 2.0 and g.max() / g.min() > 3.0
    new = rates * g
    m, flux1, _ = oracle_map(full, n, seed=101)
    assert m["counts"].sum() > 1000
    r = origin.reweight(m, rates, new)
    assert r["uncovered"] == 0.0
    full2 = sa.initFullSetup(emission=new, **SMALL)
    _, flux2, sq2 = oracle_map(full2, n, seed=202)
    scale = origin.model_mass(new, full.radii, full.energies).sum() / origin.model_mass(rates, full.radii, full.energies).sum()
    sigma = np.sqrt(r["flux_error"] ** 2 + scale * scale * sq2)
    pull = (r["flux"] - scale * flux2) / sigma
    print("reweighted %.6e direct x S'/S %.6e sigma %.3e pull %+.3f; unreweighted %.6e (%+.1f sigma)"
          % (r["flux"], scale * flux2, sigma, pull, flux1, (flux1 - scale * flux2) / sigma))
    assert abs(pull) <= 5.0
    assert abs(flux1 - scale * flux2) > 10.0 * sigma       # the test can tell: without the ratio the fluxes are far apart
    # and the wrong normalisation (the direct run taken as it is) is far off, too
    assert abs(r["flux"] - flux2) > 10.0 * sigma
