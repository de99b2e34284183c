"""CPU side of the aperture map (include/sart.h: sart_trace_histogram_aperture_device): the C-ABI tables, the Nim binding, the code
object of aperture_histogram_kernel, aperture.py on a hand-made 2 x 3 map, the binning helper of the GPU tests pinned on oracle
records against a per-ray loop (and against planted errors), and the command line's new switch."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from solaraxionraytracing_amd import _lib as L
from solaraxionraytracing_amd import aperture
from solaraxionraytracing_amd import raytracer as R
from solaraxionraytracing_amd.__main__ import build_parser, check_scan_args

from tests.aperture_binning import ApertureBinned, bin_entrance, check_map, naive_bins
from tests.binned_records import stand_in_quanta
from tests.conftest import make_setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
NEW = ("sart_set_aperture_grid", "sart_get_aperture_grid", "sart_aperture_block_len", "sart_trace_histogram_aperture_device",
       "sart_trace_histogram_aperture", "sart_finalize_aperture_device")


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
    # the struct: header, ctypes and Nim name the same fields in the same order
    m = re.search(r"typedef struct sart_aperture_grid_t \{(.*?)\} sart_aperture_grid_t;", hdr, flags=re.S)
    fields = re.findall(r"\b(nx|ny|x_min|x_max|y_min|y_max)\b", m.group(1))
    assert fields == [f for f, _ in L.ApertureGrid._fields_] == ["nx", "ny", "x_min", "x_max", "y_min", "y_max"]
    assert C.sizeof(L.ApertureGrid) == 40
    n = re.search(r"SartApertureGrid\*.*?= object\n(.*?)\nproc", nim, flags=re.S).group(1)
    assert re.findall(r"(\w+)\*", n) == fields


def test_layout_constants_agree_across_header_library_and_python():
    hdr = open(os.path.join(ROOT, "include", "sart.h")).read()
    nim = open(os.path.join(ROOT, "integration", "sart_ffi.nim")).read()
    for key, slot in L.APERTURE.items():
        assert re.search(r"SART_APERTURE_%s = %d\b" % (key, slot), hdr), key
    assert re.search(r"SART_APERTURE_N_PASSED = %d\b" % L.APERTURE_HEAD_SLOTS["N_PASSED"], hdr)
    for key, slot in L.APERTURE_HEAD_HI.items():
        assert re.search(r"SART_APERTURE_%s_HI = %d\b" % (key, slot), hdr), key
    assert re.search(r"SART_APERTURE_CELL = %d\b" % L.APERTURE_CELL, hdr) and re.search(r"SART_APERTURE_HEAD = %d\b" % L.APERTURE_HEAD, hdr)
    assert re.search(r"SartApertureHead\* = %d\b" % L.APERTURE_HEAD, nim) and re.search(r"SartApertureCell\* = %d\b" % L.APERTURE_CELL, nim)
    # the head sits at the origin head's positions, the cell is the origin cell: one fold, one finalize
    assert L.APERTURE_CELL == L.ORIGIN_CELL == 4 and L.APERTURE_HEAD == L.ORIGIN_HEAD == 8
    assert L.APERTURE == L.ORIGIN and L.APERTURE_HEAD_SLOTS == L.ORIGIN_HEAD_SLOTS and L.APERTURE_HEAD_HI == L.ORIGIN_HEAD_HI
    lib = L.load_sart()
    for nx, ny in ((1, 1), (4096, 1024), (0, 5), (-3, 5), (64, 64), (48, 20), (37, 11)):
        want = 8 + (max(nx, 0) * max(ny, 0) + 1) * 4
        assert lib.sart_aperture_block_len(nx, ny) == L.aperture_block_len(nx, ny) == R.aperture_block_len(nx, ny) == want
    assert L.APERTURE_MAX_SIDE == 4096 and L.APERTURE_MAX_CELLS == 4096 * 1024 == 1 << 22


def test_aperture_kernel_instantiations_meet_the_ray_kernel_budgets(tmp_path):
    """Exactly {not rotated, rotated} x {f64, FIXED64}, named without `trace_`; no scratch, no spills, <= 128 VGPRs, and the LDS of
    the shell and channel kernels."""
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
        if "aperture_histogram_kernel" in m.group(1):
            found[m.group(1)] = (g("private_segment_fixed_size"), g("vgpr_spill_count"), g("vgpr_count"), g("group_segment_fixed_size"))
        elif "channel_histogram_kernel" in m.group(1) or "shell_histogram_kernel" in m.group(1):
            lds[m.group(1)] = g("group_segment_fixed_size")
    want = {"_ZN4sart25aperture_histogram_kernelILi1024ELb%dELb%dEEEvNS_4HotAEPKNS_7DevBlobENS_9TraceArgsEPdNS_4HotBENS_12ApertureArgsE"
            % (r, f) for r in (0, 1) for f in (0, 1)}
    assert set(found) == want
    assert len(lds) == 8 and len(set(lds.values())) == 1
    for name, (scratch, spills, vgprs, group) in found.items():
        assert "trace_" not in name
        assert scratch == 0 and spills == 0, name
        assert vgprs <= 128, (name, vgprs)
        assert group == next(iter(lds.values())) <= 160 * 1024, (name, group)


# ---- aperture.py on a hand-made 2 x 3 map ------------------------------------------------------
def hand_map():
    """ny = 2, nx = 3 over x in [-3, 3), y in [0, 4): cell centres x = -2, 0, 2 and y = 1, 3."""
    return dict(counts=np.array([[1, 2, 0], [2, 0, 4]]), weights=np.array([[1.0, 2.0, 0.0], [4.0, 0.0, 8.0]]),
                weights_sq=np.array([[1.0, 2.0, 0.0], [8.0, 0.0, 16.0]]), outside=dict(N=3, SUM_WEIGHTS=5.0, SUM_WEIGHTS_SQ=9.0),
                x_edges=np.array([-3.0, -1.0, 1.0, 3.0]), y_edges=np.array([0.0, 2.0, 4.0]),
                head=dict(N_PASSED=12.0, SUM_WEIGHTS=20.0, SUM_WEIGHTS_SQ=36.0))


def test_split_aperture_names_the_slots():
    blk = np.arange(8 + (3 * 2 + 1) * 4, dtype=np.float64)
    a = L.split_aperture(blk, 3, 2)
    assert a["head"] == dict(N_PASSED=0.0, SUM_WEIGHTS=1.0, SUM_WEIGHTS_SQ=2.0)
    np.testing.assert_array_equal(a["counts"], [[8, 12, 16], [20, 24, 28]])      # [ny][nx], row-major as the image
    np.testing.assert_array_equal(a["weights"], a["counts"] + 1)
    np.testing.assert_array_equal(a["weights_sq"], a["counts"] + 2)
    assert a["outside"] == dict(N=32.0, SUM_WEIGHTS=33.0, SUM_WEIGHTS_SQ=34.0)
    assert L.split_aperture(blk, 2, 3)["counts"].shape == (3, 2)                # a transposed shape is another map
    with pytest.raises(AssertionError):
        L.split_aperture(blk, 3, 3)


def test_radial_profile_by_hand():
    m = hand_map()
    # centre radii: row y = 1: sqrt(5), 1, sqrt(5); row y = 3: sqrt(13), 3, sqrt(13).  Two annuli of width sqrt(13) / 2 = 1.80:
    # the first holds the one cell at r = 1, the second everything else
    p = aperture.radial_profile(m, 2)
    np.testing.assert_allclose(p["r_edges"], [0.0, math.sqrt(13) / 2, math.sqrt(13)], rtol=1e-15)
    np.testing.assert_array_equal(p["flux"], [2.0, 13.0])
    np.testing.assert_array_equal(p["counts"], [2, 7])
    np.testing.assert_allclose(p["sigma"], [math.sqrt(2.0), math.sqrt(25.0)], rtol=1e-15)
    one = aperture.radial_profile(m, 1)
    assert one["flux"][0] == m["weights"].sum() and one["counts"][0] == 9
    fine = aperture.radial_profile(m, 1000)
    assert fine["flux"].sum() == m["weights"].sum() and (fine["flux"] != 0).sum() == 3       # radii 1, sqrt(5) and sqrt(13) carry flux
    assert fine["flux"][-1] == 12.0                                                          # the largest centre radius: the last bin
    with pytest.raises(ValueError):
        aperture.radial_profile(m, 0)
    with pytest.raises(ValueError):
        aperture.radial_profile(dict(m, x_edges=m["y_edges"]), 2)


def test_reweight_by_hand():
    m = hand_map()
    ones = np.ones((2, 3))
    r = aperture.reweight(m, ones)
    assert r["flux"] == 15.0 and r["sigma"] == math.sqrt(27.0) and r["uncovered"] == 5.0 / 20.0
    r = aperture.reweight(m, ones, outside_factor=1.0)
    assert r["flux"] == 20.0 == m["head"]["SUM_WEIGHTS"] and r["sigma"] == 6.0 == math.sqrt(m["head"]["SUM_WEIGHTS_SQ"])
    # an indicator mask: an aperture stop that keeps x < 1 (the first two columns)
    mask = np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 0.0]])
    r = aperture.reweight(m, mask)
    assert r["flux"] == 7.0 and r["sigma"] == math.sqrt(11.0)
    # a random factor against math.fsum
    rng = np.random.default_rng(5)
    f = rng.random((2, 3)) * 2.0
    r = aperture.reweight(m, f, outside_factor=0.5)
    assert r["flux"] == pytest.approx(math.fsum((m["weights"] * f).ravel()) + 2.5, rel=1e-15)
    assert r["sigma"] == pytest.approx(math.sqrt(math.fsum((m["weights_sq"] * f * f).ravel()) + 9.0 * 0.25), rel=1e-15)
    # planted errors: a transposed factor is refused, a non-finite one too
    with pytest.raises(ValueError):
        aperture.reweight(m, f.T)
    with pytest.raises(ValueError):
        aperture.reweight(m, np.full((2, 3), np.nan))
    # a map without an outside cell: nothing uncovered
    bare = {k: m[k] for k in ("counts", "weights", "weights_sq")}
    assert aperture.reweight(bare, ones) == dict(flux=15.0, sigma=math.sqrt(27.0), uncovered=0.0)


def test_save_load_and_csv_round_trip(tmp_path):
    m = hand_map()
    path = aperture.save_map(str(tmp_path / "aperture_map_IAXO.npz"), m, 1000)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(["counts", "weights", "weights_sq", "outside", "x_edges", "y_edges", "n_rays", "head"])
        np.testing.assert_array_equal(z["outside"], [3.0, 5.0, 9.0])
        np.testing.assert_array_equal(z["head"], [12.0, 20.0, 36.0])
    back = aperture.load_map(path)
    assert back["outside"] == m["outside"] and back["head"] == m["head"] and back["n_rays"] == 1000.0
    for k in ("counts", "weights", "weights_sq", "x_edges", "y_edges"):
        np.testing.assert_array_equal(back[k], m[k])
    assert aperture.reweight(back, np.ones((2, 3))) == aperture.reweight(m, np.ones((2, 3)))
    rows = np.loadtxt(aperture.write_csv(str(tmp_path / "a.csv"), m), delimiter=",", skiprows=1)
    assert open(tmp_path / "a.csv").readline().strip() == "x,y,N,flux,sigma" and rows.shape == (6, 5)
    np.testing.assert_array_equal(rows[:, 0], [-2.0, 0.0, 2.0] * 2)
    np.testing.assert_array_equal(rows[:, 1], [1.0] * 3 + [3.0] * 3)
    np.testing.assert_array_equal(rows[:, 2], m["counts"].ravel())
    np.testing.assert_array_equal(rows[:, 3], m["weights"].ravel())
    np.testing.assert_array_equal(rows[:, 4], np.sqrt(m["weights_sq"]).ravel())


# ---- the binning helper of the GPU tests, on oracle records --------------------------------------
N_ORACLE, SEED, OFFSET = 300_000, 19, 512
ORACLE_CASES = {   # name: (window, passed rays, (cut window, rays outside it at 37 x 11))
    "babyiaxo_xmm": (((-352.0, 352.0), (-352.0, 352.0)), 71_939, (((0.0, 352.0), (-100.0, 250.0)), 53_163)),
    "cast_llnl": (((60.0, 106.0), (-23.0, 23.0)), 268_932, (((80.0, 106.0), (-23.0, 5.0)), 166_516)),
}


@pytest.fixture(scope="module", params=sorted(ORACLE_CASES))
def oracle_rays(request):
    from oracle.oracle import Oracle
    rec = Oracle(make_setup(request.param)).trace_records(N_ORACLE, seed=SEED, ray_id_offset=OFFSET)
    p = rec["passed"] != 0
    return request.param, rec["pointdataXBefore"][p].copy(), rec["pointdataYBefore"][p].copy(), rec["weights"][p].copy()


def test_helper_equals_a_per_ray_loop_on_oracle_records(oracle_rays):
    """The cases of tests/test_gpu_aperture.py on the CPU oracle: the passed rays, no ray within DELTA_MM of an edge on any of the
    grids, the full windows hold every ray and the cut windows leave most outside; slot for slot the helper is the per-ray loop."""
    name, x, y, w = oracle_rays
    (xr, yr), n_passed, ((cxr, cyr), n_cut) = ORACLE_CASES[name]
    assert x.size == n_passed
    q = stand_in_quanta(float(w.max()))
    for nx, ny, wx, wy in ((64, 64, xr, yr), (48, 20, xr, yr), (37, 11, cxr, cyr)):
        b = bin_entrance(x, y, w, nx, ny, wx, wy)
        assert b.n_ambiguous == 0
        n, sw, sw2 = naive_bins(x, y, w, nx, ny, wx, wy)
        sure, amb = b.cells
        np.testing.assert_array_equal(sure.count, n)
        assert not amb.count.any() and n.sum() == n_passed
        np.testing.assert_allclose(sure.w.astype(np.float64), sw, rtol=1e-15, atol=0.0)
        np.testing.assert_allclose(sure.reflect.astype(np.float64), sw2, rtol=1e-15, atol=0.0)
        assert n[-1] == (n_cut if (wx, wy) == (cxr, cyr) else 0)
        assert (n[:-1] > 0).sum() > 10 and (n[:-1] == 0).sum() > 10            # a picture: cells with and cells without rays
        check_map(b, n, sw, sw2, None, name)                                     # the loop's own sums pass as an f64 map ...
        check_map(b, n, np.rint(sw / q["weight"]) * q["weight"], np.rint(sw2 / q["weight_sq"]) * q["weight_sq"], q, name)   # ... and as FIXED64


def test_planted_errors_fail(oracle_rays):
    name, x, y, w = oracle_rays
    (xr, yr), _, _ = ORACLE_CASES[name]
    nx, ny = 48, 20
    b = bin_entrance(x, y, w, nx, ny, xr, yr)
    n, sw, sw2 = naive_bins(x, y, w, nx, ny, xr, yr)
    q = stand_in_quanta(float(w.max()))
    heavy = int(np.argmax(w))                                                    # (a ray far heavier than its cell's envelope)
    s = int(b.slot_of_ray[heavy])
    t = s + 1 if (s + 1) % nx else s - 1                                         # the cell across its x edge
    # one ray moved across an edge: counts, weights, squares each catch it on their own
    for quanta in (None, q):
        moved_n = n.copy(); moved_n[s] -= 1; moved_n[t] += 1
        with pytest.raises(AssertionError, match=" N count"):
            check_map(b, moved_n, sw, sw2, quanta, name)
        moved_w = sw.copy(); moved_w[s] -= w[heavy]; moved_w[t] += w[heavy]
        with pytest.raises(AssertionError, match="SUM_WEIGHTS w"):
            check_map(b, n, moved_w, sw2, quanta, name)
        moved_w2 = sw2.copy(); moved_w2[s] -= w[heavy] ** 2; moved_w2[t] += w[heavy] ** 2
        with pytest.raises(AssertionError, match="SUM_WEIGHTS_SQ"):
            check_map(b, n, sw, moved_w2, quanta, name)
        # one ray dropped
        less = n.copy(); less[s] -= 1
        with pytest.raises(AssertionError):
            check_map(b, less, sw, sw2, quanta, name)
    drop = np.arange(x.size) != heavy
    n1, sw1, sw21 = naive_bins(x[drop], y[drop], w[drop], nx, ny, xr, yr)
    with pytest.raises(AssertionError):
        check_map(b, n1, sw1, sw21, None, name)
    # a transposed map is another map
    bt = bin_entrance(y, x, w, nx, ny, xr, yr) if xr == yr else None
    if bt is not None:
        with pytest.raises(AssertionError):
            check_map(bt, n, sw, sw2, None, name)
    # a grid that puts rays on its edges is a bad input, not a pass
    on_edge = np.r_[x[:3], [xr[0] + (xr[1] - xr[0]) / nx * k for k in (1, 2, 3)]]
    many = ApertureBinned(on_edge, np.r_[y[:3], y[:3]], np.r_[w[:3], w[:3]], nx, ny, xr, yr)
    assert many.n_ambiguous == 3
    with pytest.raises(AssertionError, match="choose another grid"):
        bin_entrance(on_edge, np.r_[y[:3], y[:3]], np.r_[w[:3], w[:3]], nx, ny, xr, yr)


# ---- the command line --------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [["--shellBreakdown"], ["--emissionChannels", "terms"], ["--originMap"], ["--massScanMin", "0", "--massScanMax", "0.1"],
                                   ["--angularScanMin", "0", "--angularScanMax", "0.1"], ["--energyScanMin", "1", "--energyScanMax", "2"],
                                   ["--apertureBins", "0"], ["--apertureBins", "4097"], ["--apertureWindow", "0,1,2"],
                                   ["--apertureWindow", "1,0,0,1"], ["--apertureWindow", "0,1,0,nan"]])
def test_cli_refuses_aperture_map_beside_other_modes(extra, capsys):
    ap = build_parser()
    args = ap.parse_args(["--apertureMap"] + extra)
    with pytest.raises(SystemExit) as e:
        check_scan_args(ap, args)
    assert e.value.code == 2 and "--apertureMap" in capsys.readouterr().err


def test_cli_accepts_aperture_map_alone_and_with_the_test_source():
    ap = build_parser()
    check_scan_args(ap, ap.parse_args(["--apertureMap"]))
    check_scan_args(ap, ap.parse_args(["--apertureMap", "--xrayTest"]))                    # the entrance point exists for every source
    check_scan_args(ap, ap.parse_args(["--apertureMap", "--apertureBins", "37", "--apertureWindow", "0,352,-100,250"]))
    d = ap.parse_args([])
    assert d.apertureMap is False and d.apertureBins == 256 and d.apertureWindow == ""
    from solaraxionraytracing_amd.__main__ import aperture_window
    full = make_setup("babyiaxo_xmm")
    half = 1.02 * max(full.setup.all_r1[:full.setup.n_shells])
    assert aperture_window(d, full) == (-half, half, -half, half) and half > 350.0
    assert aperture_window(ap.parse_args(["--apertureWindow", "0,352,-100,250"])) == (0.0, 352.0, -100.0, 250.0)
