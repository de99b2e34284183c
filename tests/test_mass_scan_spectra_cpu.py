"""CPU side of the banded mass scan (include/sart.h: sart_trace_mass_scan_spectra): the C-ABI tables and constants, the Nim binding,
the code object of mass_scan_spectra_kernel, the band helpers of the Python layer at hand-worked numbers, and the command line's
refusals."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import solaraxionraytracing_amd as sa
from solaraxionraytracing_amd import _lib as L
from solaraxionraytracing_amd.__main__ import build_parser, check_scan_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
NEW = ("sart_mass_scan_spectra_len", "sart_trace_mass_scan_spectra_device", "sart_trace_mass_scan_spectra",
       "sart_finalize_mass_scan_spectra_device")


def test_entry_points_are_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sart.h")).read(), flags=re.S)
    nim = open(os.path.join(ROOT, "integration", "sart_ffi.nim")).read()
    lib = L.load_sart()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in L.SART_SYMBOLS, name
        assert re.search(r"proc %s\*" % name, nim), name
        assert hasattr(lib, name), name
    assert re.search(r"typedef struct sart_energy_bands_t \{ int32_t e0, width, n_bands; \} sart_energy_bands_t;", hdr)
    assert "SartEnergyBands*" in nim and "sizeof(SartEnergyBands) == 12" in nim and C.sizeof(L.EnergyBands) == 12
    assert lib.sart_abi_version() == 5
    host = L.load_host()
    assert "sart_host_axion_mass_scan_spectra" in L.SART_HOST_SYMBOLS and hasattr(host, "sart_host_axion_mass_scan_spectra")
    assert "sart_host_axion_mass_scan_spectra(" in open(os.path.join(ROOT, "include", "sart_host.h")).read()


def test_layout_constants_agree_across_headers_library_and_python():
    hdr = open(os.path.join(ROOT, "include", "sart.h")).read()
    dev = open(os.path.join(ROOT, "solaraxionraytracing_amd", "csrc", "sart_device.h")).read()
    for key, slot in list(L.MSPEC.items()) + [(k + "_HI", v) for k, v in L.MSPEC_HI.items()] + list(L.MSPEC_COUNTS.items()):
        assert re.search(r"SART_MSPEC_%s = %d\b" % (key, slot), hdr), key
    assert re.search(r"SART_MSPEC_CELL = %d\b" % L.MSPEC_CELL, hdr) and L.MSPEC_CELL == 4
    assert re.search(r"constexpr int kScanLanes = 32;", dev) and re.search(r"constexpr int kScanBandsMax = kScanLanes - 1;", dev)
    assert L.MSPEC_MAX_BANDS == 31
    lib = L.load_sart()
    for n_masses, n_bands in ((1, 1), (7, 31), (34, 31), (33, 8), (65536, 31)):
        assert lib.sart_mass_scan_spectra_len(n_masses, n_bands) == L.mass_scan_spectra_len(n_masses, n_bands) == (n_masses + 1) * (n_bands + 1) * 4
    # split: block k, cell b, slot j of a buffer that holds its own indices
    spec = np.arange(L.mass_scan_spectra_len(2, 3), dtype=np.float64)
    out = sa.split_mass_scan_spectra(spec, 2, 3)
    assert out["SUM_WEIGHTS"].shape == (2, 4) and out["SUM_WEIGHTS"][1, 2] == (1 * 4 + 2) * 4 + 0
    assert out["SUM_WEIGHTS_SQ"][0, 3] == (0 * 4 + 3) * 4 + 1 and list(out["N_ON_DETECTOR"]) == [32.0, 36.0, 40.0, 44.0]


def test_entry_points_fail_loudly_without_a_context():
    """No device, no context: every entry point returns an error and a message - none of them computes anything on the host."""
    lib, host = L.load_sart(), L.load_host()
    p = L.TraceParams()
    p.n_rays = 1000
    m = np.array([0.0, 0.008])
    b = L.EnergyBands(0, 1, 4)
    scan, spec = np.zeros(sa.mass_scan_len(2)), np.zeros(L.mass_scan_spectra_len(2, 4))
    for rc in (lib.sart_trace_mass_scan_spectra(None, C.byref(p), L.as_dp(m), 2, C.byref(b), L.as_dp(scan), L.as_dp(spec)),
               lib.sart_trace_mass_scan_spectra_device(None, C.byref(p), L.as_dp(m), 2, C.byref(b), None, None),
               lib.sart_finalize_mass_scan_spectra_device(None, C.byref(p), L.as_dp(m), 2, C.byref(b), None, None, None)):
        assert rc == L.SART_ERR_INVALID_ARGUMENT and lib.sart_last_error()
    assert not scan.any() and not spec.any()
    f = np.zeros(2)
    bf = np.zeros((2, 5))
    rc = host.sart_host_axion_mass_scan_spectra(None, L.as_dp(m), 2, 1000, 1, 0, 0, 0, 1, 4, L.as_dp(f), None, None, L.as_dp(bf), None, None)
    assert rc == L.SART_ERR_INVALID_ARGUMENT and not bf.any()


# ---- energy_bands at hand-worked edges ----------------------------------------------------------------------------
# a table of 10 points 1.0, 1.5, ..., 5.5 keV: step 0.5, cell e = [0.75 + 0.5 e, 1.25 + 0.5 e)
GRID = 1.0 + 0.5 * np.arange(10)


def test_energy_bands_at_hand_worked_edges():
    # e0 > 0: [1.75, 4.75] keV in 3 bands = cells 2 .. 7, two cells a band
    bands, edges = sa.energy_bands(GRID, 1.75, 4.75, 3)
    assert bands == (2, 2, 3) and np.allclose(edges, [1.75, 2.75, 3.75, 4.75], rtol=0, atol=1e-12)
    # the whole table in one band, in five, in ten
    assert sa.energy_bands(GRID, 0.75, 5.75, 1)[0] == (0, 10, 1)
    assert sa.energy_bands(GRID, 0.75, 5.75, 5)[0] == (0, 2, 5)
    bands, edges = sa.energy_bands(GRID, 0.75, 5.75, 10)
    assert bands == (0, 1, 10) and np.allclose(edges, 0.75 + 0.5 * np.arange(11), rtol=0, atol=1e-12)
    # a width that does not divide the range of the table: 3 bands of 3 cells from cell 1 leave cell 0 and nothing at the top ...
    assert sa.energy_bands(GRID, 1.25, 5.75, 3)[0] == (1, 3, 3)
    # ... and 2 bands of 4 cells from cell 0 leave cells 8, 9 outside
    bands, edges = sa.energy_bands(GRID, 0.75, 4.75, 2)
    assert bands == (0, 4, 2) and np.allclose(edges, [0.75, 2.75, 4.75], rtol=0, atol=1e-12)


@pytest.mark.parametrize("req", [
    (1.0, 4.0, 3),            # the lower edge is a cell centre, not a cell edge
    (0.75, 5.75, 3),          # 10 cells do not split into 3 equal bands
    (0.75, 5.75, 4),          # nor into 4
    (1.75, 2.0, 1),           # half a cell
    (0.25, 2.25, 2),          # starts below the table
    (3.75, 6.75, 3),          # ends above it
    (0.75, 5.75, 0), (0.75, 5.75, 32), (0.75, 5.75, 2.5),   # n_bands outside [1, 31], or not whole
    (4.75, 1.75, 3), (1.75, 1.75, 1), (np.nan, 4.75, 3),     # no range
])
def test_energy_bands_refuses_what_the_index_grid_cannot_represent(req):
    with pytest.raises(ValueError):
        sa.energy_bands(GRID, *req)


def test_energy_bands_refuses_a_table_that_is_no_uniform_grid():
    with pytest.raises(ValueError):
        sa.energy_bands(np.array([1.0, 1.5, 2.5, 3.0]), 0.75, 1.75, 1)
    with pytest.raises(ValueError):
        sa.energy_bands(np.array([1.0]), 0.75, 1.25, 1)


def test_band_assignment_helper_at_hand_worked_indices():
    """band_of_energy_index - what the GPU tests bin single-mass spectra and the oracle's records with - against include/sart.h's rule,
    index by index."""
    # e0 = 2, width = 3, 4 bands: window [2, 14); outside cell = 4
    got = sa.band_of_energy_index(np.arange(17), (2, 3, 4))
    assert list(got) == [4, 4, 0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4]
    # width 1: the identity inside the window
    assert list(sa.band_of_energy_index([0, 1, 2, 3, 4], (1, 1, 3))) == [3, 0, 1, 2, 3]
    # one band: everything from e0 on, up to the window's end
    assert list(sa.band_of_energy_index([0, 4, 5, 299, 300, 304, 305], (5, 300, 1))) == [1, 1, 0, 0, 0, 0, 1]
    # the X-ray test source's index n_energies follows the same rule (n_energies = 300 here)
    assert list(sa.band_of_energy_index([300], (0, 301, 1))) == [0] and list(sa.band_of_energy_index([300], (20, 3, 31))) == [31]
    # a window beyond every index: all outside
    assert list(sa.band_of_energy_index([0, 150, 300], (5000, 1, 4))) == [4, 4, 4]
    # the multiply-shift of the kernel (sart_device.h: ScanMass::aux) gives the same bands for every index a table can hold
    for e0, width, n_bands in ((2, 3, 4), (20, 3, 31), (0, 301, 1), (0, 1, 31), (7, 97, 31), (0, 2111, 31)):
        n_idx = 65536
        w = min(width, n_idx)
        mul = ((1 << 31) + w - 1) // w
        e = np.arange(n_idx, dtype=np.int64)
        d = (e - e0) % (1 << 32)
        cell = np.where(d < n_bands * w, ((2 * d + 1) * mul) >> 32, n_bands)
        assert np.array_equal(cell, sa.band_of_energy_index(e, (e0, width, n_bands))), (e0, width, n_bands)


# ---- the code object ------------------------------------------------------------------------------------------------
def test_kernels_meet_the_ray_kernel_budgets(tmp_path):
    """mass_scan_spectra_kernel: no scratch, <= 128 VGPRs, LDS within 160 KB, and the argument offsets of trace_histogram_kernel (it
    re-reads its arguments at those) - for the four scan variants in f64 and FIXED64."""
    obj = tmp_path / "sart_kernels.o"
    shutil.copy(os.path.join(ROOT, "solaraxionraytracing_amd", "csrc", "build", "sart_kernels.o"), obj)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", str(obj)], check=True, capture_output=True, cwd=tmp_path)
    dev = [f for f in os.listdir(tmp_path) if "amdgcn" in f]
    assert len(dev) == 1, dev
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(tmp_path / dev[0])], capture_output=True, text=True,
                           check=True).stdout
    want = (C.c_int32 * 8)()
    L.load_sart().sart_internal_kernarg_layout(want)
    seen = folds = 0
    for k in re.split(r"\n  - \.a", notes):
        m = re.search(r"\.name:\s+(\S+)", k)
        if not m:
            continue
        g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, k).group(1))
        if "mass_scan_spectra_kernel" in m.group(1):
            assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0, m.group(1)
            assert g("vgpr_count") <= 128, (m.group(1), g("vgpr_count"))
            assert 160 * 1024 - 4096 < g("group_segment_fixed_size") <= 160 * 1024, g("group_segment_fixed_size")
            args = re.findall(r"\.offset:\s+(\d+)\s+\.size:\s+(\d+)\s+\.value_kind:\s+(\w+)", k)
            explicit = [(int(o), int(sz)) for o, sz, kind in args if not kind.startswith("hidden")]
            assert [o for o, _ in explicit] == list(want[:6]), (m.group(1), explicit, list(want))
            assert explicit[-1][0] + explicit[-1][1] <= want[6]
            seen += 1
        if "fold_scan_bands_kernel" in m.group(1) or "finalize_scan_bands_kernel" in m.group(1):
            assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0, m.group(1)
            folds += 1
    assert seen == 8 and folds == 3


# ---- the command line -------------------------------------------------------------------------------------------------
def _parse(argv):
    ap = build_parser()
    args = ap.parse_args(argv)
    check_scan_args(ap, args)
    return args


def test_cli_accepts_the_band_switches():
    a = _parse(["--massScanMin", "0", "--massScanMax", "0.02", "--massScanBands", "8", "--massScanBandMin", "1", "--massScanBandMax", "9"])
    assert (a.massScanBands, a.massScanBandMin, a.massScanBandMax) == (8, 1.0, 9.0)
    assert _parse([]).massScanBands == 0


@pytest.mark.parametrize("argv", [
    ["--massScanBands", "8"],                                                                # no mass scan
    ["--massScanBandMin", "1", "--massScanBandMax", "9", "--massScanMin", "0", "--massScanMax", "0.02"],   # a window without bands
    ["--massScanBands", "8", "--massScanMin", "0", "--massScanMax", "0.02", "--angularScanMin", "0", "--angularScanMax", "0.1"],
    ["--massScanBands", "8", "--xrayTest", "--energyScanMin", "1", "--energyScanMax", "8"],
    ["--massScanBands", "8", "--massScanMin", "0", "--massScanMax", "0.02", "--xrayTest", "--energyScanMin", "1", "--energyScanMax", "8"],
    ["--massScanBands", "32", "--massScanMin", "0", "--massScanMax", "0.02"],
    ["--massScanBands", "-1", "--massScanMin", "0", "--massScanMax", "0.02"],
    ["--massScanBands", "8", "--massScanMin", "0", "--massScanMax", "0.02", "--massScanBandMin", "1"],
    ["--massScanBands", "8", "--massScanMin", "0", "--massScanMax", "0.02", "--massScanBandMin", "5", "--massScanBandMax", "1"],
])
def test_cli_refuses_bands_without_a_mass_scan_or_beside_another_scan(argv):
    with pytest.raises(SystemExit) as e:
        _parse(argv)
    assert e.value.code == 2


def test_cli_refuses_bands_in_the_vacuum_stage_and_off_the_index_grid(tmp_path):
    """Exit 2 before any GPU work and before anything is written."""
    from solaraxionraytracing_amd.__main__ import main
    out = tmp_path / "o"
    with pytest.raises(SystemExit) as e:     # the default setup is the vacuum stage
        main(["--massScanMin", "0", "--massScanMax", "0.02", "--massScanBands", "8", "--outpath", str(out)])
    assert e.value.code == 2 and not out.exists()
    sample = open(os.path.join(ROOT, "tools", "make_nim_parity_kit.py")).read()
    cfg = tmp_path / "config.toml"
    cfg.write_text(sample.split('CONFIG_TEMPLATE = """')[1].split('"""')[0] % ("BabyIAXO", "InGridIAXO", "gas", "XMM"))
    with pytest.raises(SystemExit) as e:     # gas stage, but 1.0 keV is no cell edge of the energy table
        main(["--config", str(cfg), "--massScanMin", "0", "--massScanMax", "0.02", "--massScanBands", "7", "--massScanBandMin", "1.0",
              "--massScanBandMax", "8.0001", "--outpath", str(out)])
    assert e.value.code == 2 and not out.exists()
