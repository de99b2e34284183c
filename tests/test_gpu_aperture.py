"""Aperture map of the histogram trace (include/sart.h: sart_trace_histogram_aperture_device) on the MI355X box.

Demanded here:
  * the accumulator of an aperture launch equals sart_trace_histogram_device's for the same params and ray ids, raw int64 slot for slot
    in SART_ACCUM_FIXED64 (against the generic kernel variants, which the aperture kernel is built on), spectra and flux-only included;
  * a host mirror (tests/aperture_binning.py) built from the passed rays' own pointdataXBefore / pointdataYBefore / weights columns:
    N per cell exact, every sure cell without a ray 0, no ray left out, the sums inside the envelope of tests/binned_records.py, the
    outside cell held to the same mirror - on 64 x 64, on 48 x 20 (nx != ny: a transposed index) and on a window that cuts the pupil;
  * conservation as Python integers: cells + outside = head = the accumulator's scalars;
  * 2 x 2 and 1 x 1 grids, where a quarter of a wave's lanes, or all of them, add to one cell in one instruction;
  * splits and shards give the same integers; f64 and finalized FIXED64 agree; refused calls change nothing; crafted raw blocks through
    sart_finalize_aperture_device; --apertureMap end to end; one context through aperture, shells, origin, plain, aperture."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import solaraxionraytracing_amd as sa
from solaraxionraytracing_amd import _lib as L
from solaraxionraytracing_amd import aperture

from tests.aperture_binning import bin_entrance, check_map
from tests.conftest import SMALL, make_setup

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO40 = 2 ** L.FIXED_LIMB_BITS
LIMIT = 1 << 62
N_RADIAL = 1000
N_RAYS = 300_000
SEED, OFFSET = 19, 512
SENT, SENTINEL = 64, 0x5A5A5A5A5A5A5A5A
HEAD, CELL = L.APERTURE_HEAD, L.APERTURE_CELL
A_N, A_W, A_W2 = L.APERTURE["N"], L.APERTURE["SUM_WEIGHTS"], L.APERTURE["SUM_WEIGHTS_SQ"]
H_N, H_W, H_W2 = (L.APERTURE_HEAD_SLOTS[k] for k in ("N_PASSED", "SUM_WEIGHTS", "SUM_WEIGHTS_SQ"))
H_W_HI, H_W2_HI = L.APERTURE_HEAD_HI["SUM_WEIGHTS"], L.APERTURE_HEAD_HI["SUM_WEIGHTS_SQ"]

BABY = ((-352.0, 352.0), (-352.0, 352.0))
LLNL = ((60.0, 106.0), (-23.0, 23.0))     # the sector sits off the frame's origin: a rectangle, not a half-width
# name: (window, (cut window, share of the passed rays outside it on the CPU oracle: tests/test_aperture_cpu.py))
CASES = {"babyiaxo_xmm": (BABY, (((0.0, 352.0), (-100.0, 250.0)), 53_163 / 71_939)),
         "babyiaxo_xmm_gas": (BABY, (((0.0, 352.0), (-100.0, 250.0)), 53_163 / 71_939)),
         "babyiaxo_xmm_rot": (BABY, (((0.0, 352.0), (-100.0, 250.0)), None)),
         "babyiaxo_xmm_xray": (BABY, (((0.0, 352.0), (-100.0, 250.0)), None)),
         "cast_llnl": (LLNL, (((80.0, 106.0), (-23.0, 5.0)), 166_516 / 268_932))}


def setup_of(name):
    if name == "babyiaxo_xmm_rot":
        full = make_setup("babyiaxo_xmm")
        full.setup.telescope_turned_x_deg, full.setup.telescope_turned_y_deg = 0.01, 0.03
        return full
    return make_setup(name)


class Tracer:
    """A RayTracer with SART_FORCE_GENERIC set while it is created (the aperture kernel is the generic histogram kernel's twin)."""

    def __init__(self, full, generic=True):
        if generic:
            os.environ["SART_FORCE_GENERIC"] = "1"
        try:
            self.rt = sa.RayTracer(full)
        finally:
            os.environ.pop("SART_FORCE_GENERIC", None)

    def __enter__(self):
        return self.rt

    def __exit__(self, *exc):
        self.rt.close()


def params(rt, n, seed, off=0, spectra=True, image_n=256, accumulate=False):
    return rt.aperture_params(n, seed, off, image_n=image_n, spectra=spectra, n_radial_bins=N_RADIAL, accumulate=accumulate)


def acc_len(rt, p):
    n_img = p.image_nx * p.image_ny
    return n_img + L.SART_ACC_COUNT + ((2 * p.n_radial_bins + 3 * (rt.full.energies.size + 1)) if p.spectra else 0)


def zeros(torch, n, dtype):
    """A zero-filled device buffer whose fill has FINISHED (torch fills on its own stream, the library launches on the context's)."""
    t = torch.zeros(n, dtype=dtype, device="cuda")
    torch.cuda.synchronize()
    return t


def grid(rt, nx, ny, window):
    (x0, x1), (y0, y1) = window
    rt.set_aperture_grid(nx, ny, x0, x1, y0, y1)
    assert rt.aperture_grid() == dict(nx=nx, ny=ny, x_min=x0, x_max=x1, y_min=y0, y_max=y1)
    assert rt.aperture_block_len() == L.aperture_block_len(nx, ny)


def run_aperture(rt, torch, pieces, seed, spectra=True, image_n=256, dtype=None):
    """Raw accumulator and aperture block of one accumulation over the (lo, hi) ray-id pieces, on the context's grid."""
    dtype = dtype or torch.int64
    p0 = params(rt, 1, seed, spectra=spectra, image_n=image_n)
    acc = zeros(torch, acc_len(rt, p0), dtype)
    blk = zeros(torch, rt.aperture_block_len(), dtype)
    for lo, hi in pieces:
        p = params(rt, hi - lo, seed, lo, spectra, image_n, accumulate=True)
        rt.trace_aperture_device(p, acc.data_ptr(), blk.data_ptr())
    rt.synchronize()
    return acc.cpu().numpy(), blk.cpu().numpy()


def run_hist(rt, torch, n, seed, off=0, spectra=True, image_n=256):
    p = params(rt, n, seed, off, spectra, image_n)
    acc = zeros(torch, acc_len(rt, p), torch.int64)
    rt.trace_histogram_device(p, acc.data_ptr())
    rt.synchronize()
    return acc.cpu().numpy()


def split(blk, nx, ny):
    """(head [8], slots [nx ny + 1][4]: the grid's cells row-major, then the outside cell) of a raw block."""
    assert blk.size == L.aperture_block_len(nx, ny)
    return blk[:HEAD], blk[HEAD:].reshape(nx * ny + 1, CELL)


def limbs(lo, hi):
    return int(hi) * TWO40 + int(lo)


def isum(a):
    """Exact sum of an int64 array as a Python int."""
    a = np.asarray(a).reshape(-1)
    return sum(int(v) for v in a[a != 0])


def scalars_of(acc, image_n=256):
    return acc[image_n * image_n:image_n * image_n + L.SART_ACC_COUNT]


def assert_conserved(head, slots, sc):
    """cells + outside = head = the accumulator's scalars, as Python integers; limbs normalised; reserved slots 0."""
    assert 0 <= head[H_W] < TWO40 and 0 <= head[H_W2] < TWO40
    assert head[3] == 0 and head[6] == 0 and head[7] == 0 and not slots[:, 3].any()
    n, w, w2 = int(head[H_N]), limbs(head[H_W], head[H_W_HI]), limbs(head[H_W2], head[H_W2_HI])
    assert isum(slots[:, A_N]) == n == int(sc[L.ACC["N_PASSED"]])
    assert isum(slots[:, A_W]) == w == limbs(sc[L.ACC["SUM_WEIGHTS"]], sc[L.ACC_HI["SUM_WEIGHTS"]])
    assert isum(slots[:, A_W2]) == w2 == limbs(sc[L.ACC["SUM_WEIGHTS_SQ"]], sc[L.ACC_HI["SUM_WEIGHTS_SQ"]])
    return n, w, w2


def passed_rays(rt, n, seed, off):
    """The passed rays of [off, off + n): entrance point and weight, from the columns of the same ids."""
    cols, counts = rt.trace_columns(n, ("ray_id", "pointdataXBefore", "pointdataYBefore", "weights"), seed=seed, ray_id_offset=off)
    assert counts["n_passed"] == cols["ray_id"].size > 100
    assert np.all((cols["ray_id"] >= off) & (cols["ray_id"] < off + n)) and np.all(np.diff(cols["ray_id"].astype(np.int64)) > 0)
    return cols["pointdataXBefore"].copy(), cols["pointdataYBefore"].copy(), cols["weights"].copy()


# ---- 1: the accumulator ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_fixed64_accumulator_equals_the_histogram(name):
    import torch
    window = CASES[name][0]
    with Tracer(setup_of(name)) as rt:
        rt.set_accumulation_mode("fixed64")
        grid(rt, 64, 64, window)
        for spectra, image_n in ((True, 256), (False, 0)):
            ref = run_hist(rt, torch, N_RAYS, 7, 13, spectra, image_n)
            acc, blk = run_aperture(rt, torch, [(13, 13 + N_RAYS)], 7, spectra, image_n)
            np.testing.assert_array_equal(acc, ref)
            head, slots = split(blk, 64, 64)
            n, _, _ = assert_conserved(head, slots, scalars_of(acc, image_n))
            assert n > 100


# ---- 2 + 3: the mirror and the conservation laws -------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_mirror_and_conservation(name):
    import torch
    window, (cut, cut_share) = CASES[name]
    with Tracer(setup_of(name)) as rt:
        x, y, w = passed_rays(rt, N_RAYS, SEED, OFFSET)
        for nx, ny, win in ((64, 64, window), (48, 20, window), (37, 11, cut)):
            what = "%s %dx%d" % (name, nx, ny)
            b = bin_entrance(x, y, w, nx, ny, *win)          # (more than MAX_AMBIGUOUS rays on an edge: a bad input, it asserts)
            grid(rt, nx, ny, win)
            rt.set_accumulation_mode("fixed64")
            acc, blk = run_aperture(rt, torch, [(OFFSET, OFFSET + N_RAYS)], SEED)
            q = rt.fixed_quanta()
            rt.set_accumulation_mode("f64")
            acc_f, blk_f = run_aperture(rt, torch, [(OFFSET, OFFSET + N_RAYS)], SEED, dtype=torch.float64)
            head, slots = split(blk, nx, ny)
            n, _, _ = assert_conserved(head, slots, scalars_of(acc))
            assert n == w.size                                                    # no ray left out
            outside_share = int(slots[-1, A_N]) / n
            print(what, "passed %d, ambiguous %d, outside %d (%.4f), cells without a ray %d of %d"
                  % (n, b.n_ambiguous, int(slots[-1, A_N]), outside_share, int((slots[:-1, A_N] == 0).sum()), nx * ny))
            check_map(b, slots[:, A_N], slots[:, A_W].astype(np.float64) * q["weight"], slots[:, A_W2].astype(np.float64) * q["weight_sq"],
                      q, what + " fixed64")
            if win is window:
                assert slots[-1, A_N] == 0 and not slots[-1].any()                # the full window holds the whole pupil
            else:
                assert slots[-1, A_N] > 0.3 * n                                   # the cut window leaves much of it outside
                if cut_share is not None:
                    assert abs(outside_share - cut_share) < 0.01
            assert (slots[:-1, A_N] == 0).sum() > 10 and (slots[:-1, A_N] > 0).sum() > 10
            # f64: the same mirror, its own envelope; the head is the scalars' through a second fold tree
            head_f, slots_f = split(blk_f, nx, ny)
            check_map(b, slots_f[:, A_N], slots_f[:, A_W], slots_f[:, A_W2], None, what + " f64")
            np.testing.assert_array_equal(slots_f[:, A_N], slots[:, A_N].astype(np.float64))
            assert not slots_f[:, 3].any() and not head_f[3:].any()
            sc_f = scalars_of(acc_f)
            assert head_f[H_N] == n == sc_f[L.ACC["N_PASSED"]]
            for hk, key in ((H_W, "SUM_WEIGHTS"), (H_W2, "SUM_WEIGHTS_SQ")):
                assert head_f[hk] == pytest.approx(sc_f[L.ACC[key]], rel=1e-12)
            assert slots_f[:, A_W].sum() == pytest.approx(head_f[H_W], rel=1e-12)


# ---- 4: grids where lanes collide -----------------------------------------------------------------
@pytest.mark.parametrize("side", [2, 1])
@pytest.mark.parametrize("name", ["babyiaxo_xmm", "babyiaxo_xmm_rot"])
def test_tiny_grids_where_lanes_of_one_wave_share_a_cell(name, side):
    """2 x 2: a quarter of the passed rays per cell (the pupil is symmetric about the axis), 16 lanes of a wave of 64 passed rays in
    one instruction; 1 x 1: all of them."""
    import torch
    n, seed, off = 100_000, 29, 1024
    with Tracer(setup_of(name)) as rt:
        x, y, w = passed_rays(rt, n, seed, off)
        b = bin_entrance(x, y, w, side, side, *BABY)
        grid(rt, side, side, BABY)
        rt.set_accumulation_mode("fixed64")
        acc, blk = run_aperture(rt, torch, [(off, off + n)], seed)
        q = rt.fixed_quanta()
        rt.set_accumulation_mode("f64")
        _, blk_f = run_aperture(rt, torch, [(off, off + n)], seed, dtype=torch.float64)
    head, slots = split(blk, side, side)
    n_passed, _, _ = assert_conserved(head, slots, scalars_of(acc))
    assert n_passed == w.size and slots[-1, A_N] == 0
    check_map(b, slots[:, A_N], slots[:, A_W].astype(np.float64) * q["weight"], slots[:, A_W2].astype(np.float64) * q["weight_sq"], q, name)
    _, slots_f = split(blk_f, side, side)
    check_map(b, slots_f[:, A_N], slots_f[:, A_W], slots_f[:, A_W2], None, name + " f64")
    share = slots[:-1, A_N].max() / n_passed
    print(name, side, "busiest cell: %.1f lanes of 64" % (64 * share))
    if side == 1:
        assert share == 1.0
    else:
        assert 0.23 < share < 0.28      # 0.25 on the oracle; the four shares are binomial, sigma 0.003 at 2e4 passed rays


# ---- 5: splits, shards and modes ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["babyiaxo_xmm_gas", "cast_llnl"])
def test_splits_and_shards_give_the_same_integers(name):
    import torch
    n, seed = N_RAYS, 5
    with Tracer(setup_of(name)) as rt:
        rt.set_accumulation_mode("fixed64")
        grid(rt, 48, 20, CASES[name][0])
        a1, b1 = run_aperture(rt, torch, [(0, n)], seed)
        a2, b2 = run_aperture(rt, torch, [(0, 77_777), (77_777, n)], seed)
        a3, b3 = run_aperture(rt, torch, [(0, 123_456)], seed)
        a4, b4 = run_aperture(rt, torch, [(123_456, n)], seed)
    np.testing.assert_array_equal(a1, a2)
    np.testing.assert_array_equal(b1, b2)
    # shards summed as int64 (what an all-reduce of the raw buffers does); the limbs are renormalised by value, not slot for slot
    h1, c1 = split(b1, 48, 20)
    h34, c34 = split(b3 + b4, 48, 20)
    np.testing.assert_array_equal(c1, c34)
    assert h1[H_N] == h34[H_N] > 1000
    assert limbs(h1[H_W], h1[H_W_HI]) == limbs(h34[H_W], h34[H_W_HI]) and limbs(h1[H_W2], h1[H_W2_HI]) == limbs(h34[H_W2], h34[H_W2_HI])


@pytest.mark.parametrize("name", ["babyiaxo_xmm", "cast_llnl", "babyiaxo_xmm_xray"])
def test_f64_and_finalized_fixed64_agree(name):
    window, (cut, _) = CASES[name]
    with Tracer(setup_of(name)) as rt:
        grid(rt, 37, 11, cut)
        img_f, s_f, sp_f, a_f = rt.trace_aperture(N_RAYS, seed=9)
        rt.set_accumulation_mode("fixed64")
        img_x, s_x, sp_x, a_x = rt.trace_aperture(N_RAYS, seed=9)     # (its finalize checks the conservation laws on the device)
        q = rt.fixed_quanta()
    # FIXED64 rounds every ray's contribution to its quantum (<= q / 2 each): a cell of k rays agrees to k q / 2 in absolute terms
    np.testing.assert_array_equal(a_f["counts"], a_x["counts"])
    assert a_f["counts"].shape == (11, 37) and a_f["outside"]["N"] == a_x["outside"]["N"] > 0
    k = a_f["counts"]
    assert np.all(np.abs(a_x["weights"] - a_f["weights"]) <= 1e-11 * a_f["weights"] + 0.5 * q["weight"] * k)
    assert np.all(np.abs(a_x["weights_sq"] - a_f["weights_sq"]) <= 1e-11 * a_f["weights_sq"] + 0.5 * q["weight_sq"] * k)
    ko = a_f["outside"]["N"]
    assert abs(a_x["outside"]["SUM_WEIGHTS"] - a_f["outside"]["SUM_WEIGHTS"]) <= 1e-11 * a_f["outside"]["SUM_WEIGHTS"] + 0.5 * q["weight"] * ko
    assert a_x["head"]["N_PASSED"] == a_f["head"]["N_PASSED"] == s_f["N_PASSED"] == k.sum() + ko
    for key in ("SUM_WEIGHTS", "SUM_WEIGHTS_SQ"):
        assert a_x["head"][key] == s_x[key]                                        # the same integers, the same quantum
        assert a_f["head"][key] == pytest.approx(s_f[key], rel=1e-12)
        assert a_x["head"][key] == pytest.approx(a_f["head"][key], rel=1e-9)
    assert a_x["weights"].sum() + a_x["outside"]["SUM_WEIGHTS"] == pytest.approx(s_x["SUM_WEIGHTS"], rel=1e-12)
    r = aperture.reweight(a_x, np.ones_like(a_x["weights"]), outside_factor=1.0)
    assert r["flux"] == pytest.approx(s_x["SUM_WEIGHTS"], rel=1e-12) and r["sigma"] == pytest.approx(np.sqrt(s_x["SUM_WEIGHTS_SQ"]), rel=1e-12)
    assert r["uncovered"] == pytest.approx(a_x["outside"]["SUM_WEIGHTS"] / s_x["SUM_WEIGHTS"], rel=1e-12)
    assert img_x.shape == img_f.shape == (256, 256) and sp_x["energy_counts"].sum() == sp_f["energy_counts"].sum() == s_x["N_PASSED"]


# ---- 6: error paths --------------------------------------------------------------------------------------
def test_refused_calls_leave_the_context_unchanged():
    """After EVERY refused call: the setup bytes, the grid and a following launch are what they were, and nothing was written."""
    import torch
    full = setup_of("babyiaxo_xmm")
    n, seed = 50_000, 4
    with Tracer(full) as rt:
        lib, h = rt.lib, rt.handle
        rt.set_accumulation_mode("fixed64")
        p_good = params(rt, n, seed)
        acc = zeros(torch, acc_len(rt, p_good), torch.int64)
        blk = zeros(torch, L.aperture_block_len(48, 20), torch.int64)

        def trace_rc(p, a, b):
            return lib.sart_trace_histogram_aperture_device(h, C.byref(p), C.c_void_p(a), C.c_void_p(b))

        def fin_rc(p, a, b):
            return lib.sart_finalize_aperture_device(h, C.byref(p) if p is not None else None, C.c_void_p(a), C.c_void_p(b))

        # no grid yet: NOT_READY from every entry, and from the getter
        g = L.ApertureGrid()
        assert lib.sart_get_aperture_grid(h, C.byref(g)) == L.SART_ERR_NOT_READY and b"aperture grid" in lib.sart_last_error()
        assert trace_rc(p_good, acc.data_ptr(), blk.data_ptr()) == L.SART_ERR_NOT_READY and b"aperture grid" in lib.sart_last_error()
        assert fin_rc(p_good, blk.data_ptr(), blk.data_ptr()) == L.SART_ERR_NOT_READY and b"aperture grid" in lib.sart_last_error()
        assert lib.sart_trace_histogram_aperture(h, C.byref(p_good), None, None, None, None) == L.SART_ERR_NOT_READY
        with pytest.raises(L.SartError) as e:
            rt.trace_aperture(1000)
        assert e.value.code == L.SART_ERR_NOT_READY
        with pytest.raises(L.SartError) as e:
            rt.aperture_block_len()
        assert e.value.code == L.SART_ERR_NOT_READY
        ref = run_hist(rt, torch, n, seed)

        grid(rt, 48, 20, BABY)
        s0 = L.Setup()
        L.check(lib.sart_get_setup(h, C.byref(s0)))
        g0 = rt.aperture_grid()
        a0, b0 = run_aperture(rt, torch, [(0, n)], seed)
        np.testing.assert_array_equal(a0, ref)

        def refused(rc, code=L.SART_ERR_INVALID_ARGUMENT, *words):
            msg = lib.sart_last_error()
            assert rc == code, (rc, msg)
            for w in words:
                assert w in msg, (w, msg)
            s1 = L.Setup()
            L.check(lib.sart_get_setup(h, C.byref(s1)))
            assert bytes(s0) == bytes(s1) and rt.aperture_grid() == g0
            a1, b1 = run_aperture(rt, torch, [(0, n)], seed)
            np.testing.assert_array_equal(a1, a0)
            np.testing.assert_array_equal(b1, b0)

        refused(trace_rc(p_good, 0, blk.data_ptr()), L.SART_ERR_INVALID_ARGUMENT, b"NULL")
        refused(trace_rc(p_good, acc.data_ptr(), 0), L.SART_ERR_INVALID_ARGUMENT, b"NULL")
        refused(lib.sart_trace_histogram_aperture_device(h, None, C.c_void_p(acc.data_ptr()), C.c_void_p(blk.data_ptr())))
        refused(lib.sart_trace_histogram_aperture_device(None, C.byref(p_good), C.c_void_p(acc.data_ptr()), C.c_void_p(blk.data_ptr())))
        refused(fin_rc(p_good, 0, blk.data_ptr()))
        refused(fin_rc(p_good, blk.data_ptr(), 0))
        refused(fin_rc(None, blk.data_ptr(), blk.data_ptr()))
        refused(lib.sart_trace_histogram_aperture(h, None, None, None, None, None))
        refused(lib.sart_set_aperture_grid(h, None), L.SART_ERR_INVALID_ARGUMENT, b"NULL")
        refused(lib.sart_set_aperture_grid(None, C.byref(L.ApertureGrid(4, 4, 0.0, 1.0, 0.0, 1.0))), L.SART_ERR_INVALID_ARGUMENT, b"NULL")
        refused(lib.sart_get_aperture_grid(h, None), L.SART_ERR_INVALID_ARGUMENT, b"NULL")
        nan, inf = float("nan"), float("inf")
        for bad, word in (((0, 4, 0.0, 1.0, 0.0, 1.0), b"[1, 4096]"), ((4097, 4, 0.0, 1.0, 0.0, 1.0), b"[1, 4096]"),
                          ((4, 0, 0.0, 1.0, 0.0, 1.0), b"[1, 4096]"), ((4, 4097, 0.0, 1.0, 0.0, 1.0), b"[1, 4096]"),
                          ((-1, 4, 0.0, 1.0, 0.0, 1.0), b"[1, 4096]"),
                          ((2049, 2048, 0.0, 1.0, 0.0, 1.0), b"2^22"), ((4096, 1025, 0.0, 1.0, 0.0, 1.0), b"2^22"),
                          ((4, 4, 1.0, 1.0, 0.0, 1.0), b"range"), ((4, 4, 2.0, 1.0, 0.0, 1.0), b"range"), ((4, 4, 0.0, 1.0, 1.0, 0.5), b"range"),
                          ((4, 4, nan, 1.0, 0.0, 1.0), b"range"), ((4, 4, 0.0, 1.0, 0.0, nan), b"range"), ((4, 4, 0.0, inf, 0.0, 1.0), b"range"),
                          ((4, 4, -inf, 1.0, 0.0, 1.0), b"range"), ((4, 4, -1e308, 1e308, 0.0, 1.0), b"range")):
            refused(lib.sart_set_aperture_grid(h, C.byref(L.ApertureGrid(*bad))), L.SART_ERR_INVALID_ARGUMENT, word)
            with pytest.raises(L.SartError):
                rt.set_aperture_grid(*bad)
        for field, value, word in (("image_nx", -1, b"image"), ("image_nx", 0, b"image"), ("image_x_max", -1.0, b"image"),
                                   ("n_radial_bins", 0, b"spectra"), ("radial_max", 0.0, b"spectra")):
            p = params(rt, n, seed)
            setattr(p, field, value)
            refused(trace_rc(p, acc.data_ptr(), blk.data_ptr()), L.SART_ERR_INVALID_ARGUMENT, word)
            refused(fin_rc(p, blk.data_ptr(), blk.data_ptr()), L.SART_ERR_INVALID_ARGUMENT, word)
            refused(lib.sart_trace_histogram_aperture(h, C.byref(p), None, None, None, None), L.SART_ERR_INVALID_ARGUMENT, word)
        rt.synchronize()
        assert int(acc.abs().sum()) == 0 and int(blk.abs().sum()) == 0     # no refused call wrote to the caller's buffers
        # the largest shapes are accepted (and replace the grid)
        for ok in ((4096, 1024, 0.0, 1.0, 0.0, 1.0), (1, 1, -1.0, 1.0, -1.0, 1.0), (2048, 2048, 0.0, 1.0, 0.0, 1.0)):
            rt.set_aperture_grid(*ok)
            assert rt.aperture_block_len() == 8 + (ok[0] * ok[1] + 1) * 4
    # a context without a setup: NOT_READY
    lib = L.load_sart()
    h = C.c_void_p()
    L.check(lib.sart_create(0, C.byref(h)))
    try:
        L.check(lib.sart_set_aperture_grid(h, C.byref(L.ApertureGrid(4, 4, 0.0, 1.0, 0.0, 1.0))))
        acc = zeros(torch, L.SART_ACC_COUNT, torch.float64)
        blk = zeros(torch, L.aperture_block_len(4, 4), torch.float64)
        p = L.TraceParams()
        C.memmove(C.byref(p), C.byref(p_good), C.sizeof(p))
        p.image_nx = p.image_ny = p.spectra = 0
        rc = lib.sart_trace_histogram_aperture_device(h, C.byref(p), C.c_void_p(acc.data_ptr()), C.c_void_p(blk.data_ptr()))
        assert rc == L.SART_ERR_NOT_READY and b"setup" in lib.sart_last_error()
        torch.cuda.synchronize()
        assert float(acc.abs().sum()) == 0.0 and float(blk.abs().sum()) == 0.0
    finally:
        lib.sart_destroy(h)


# ---- 7: crafted raw blocks ----------------------------------------------------------------------------------
def upload(torch, arr):
    arr = np.asarray(arr, dtype=np.int64).reshape(-1)
    buf = np.full(arr.size + SENT, SENTINEL, dtype=np.int64)
    buf[:arr.size] = arr
    d = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    return d


def fetch(d, n):
    h = d.cpu().numpy()
    assert h.size == n + SENT and (h[n:] == SENTINEL).all(), "the slots behind the buffer were written"
    return h[:n].copy()


def finalize(rt, torch, p, raw, in_place=False):
    d_raw = upload(torch, raw)
    d_out = d_raw if in_place else upload(torch, np.full(raw.size, SENTINEL, dtype=np.int64))
    rt.finalize_aperture_device(p, d_raw.data_ptr(), None if in_place else d_out.data_ptr())
    err = None
    try:
        rt.synchronize()
    except L.SartError as e:
        err = e
        assert e.code == L.SART_ERR_ACCUMULATOR, str(e)
    out = fetch(d_out, raw.size).view(np.float64)
    if not in_place:
        assert np.array_equal(fetch(d_raw, raw.size), raw)
    return out, err


def crafted_block(rng, nx, ny):
    """A consistent raw block: a third of the cells and the outside cell occupied, by rays of 2^13 .. 2^35 quanta (limbs in use), the
    head their sums."""
    slots = np.zeros((nx * ny + 1, CELL), dtype=np.int64)
    occ = rng.random(nx * ny + 1) < 0.33
    occ[0] = occ[-1] = occ[-2] = True
    k = int(occ.sum())
    slots[occ, A_N] = rng.integers(1, 1000, k)
    slots[occ, A_W] = slots[occ, A_N] * rng.integers(1 << 13, 1 << 35, k)
    slots[occ, A_W2] = slots[occ, A_N] * rng.integers(1 << 7, 1 << 33, k)
    head = np.zeros(HEAD, dtype=np.int64)
    w, w2 = isum(slots[:, A_W]), isum(slots[:, A_W2])
    head[H_N] = isum(slots[:, A_N])
    head[H_W], head[H_W_HI] = w % TWO40, w // TWO40
    head[H_W2], head[H_W2_HI] = w2 % TWO40, w2 // TWO40
    assert head[H_W_HI] > 0 and head[H_W2_HI] > 0
    return np.concatenate([head, slots.reshape(-1)])


def test_finalize_on_crafted_blocks():
    import torch
    nx, ny = 37, 11
    with Tracer(setup_of("babyiaxo_xmm")) as rt:
        rt.set_accumulation_mode("fixed64")
        acc = zeros(torch, L.SART_ACC_COUNT, torch.int64)
        rt.trace_histogram_device(rt.trace_params(1000, seed=3, image_n=0), acc.data_ptr())    # freezes the quanta
        rt.synchronize()
        q = rt.fixed_quanta()
        grid(rt, nx, ny, BABY)
        p = params(rt, 1, 3, spectra=False, image_n=0)
        base = crafted_block(np.random.default_rng(41), nx, ny)
        assert base.size == rt.aperture_block_len()

        def want_of(raw):
            out = np.zeros(raw.size)
            c = raw[HEAD:].reshape(-1, CELL)
            o = out[HEAD:].reshape(-1, CELL)
            o[:, A_N] = c[:, A_N]
            o[:, A_W] = c[:, A_W].astype(np.float64) * q["weight"]
            o[:, A_W2] = c[:, A_W2].astype(np.float64) * q["weight_sq"]
            out[H_N] = raw[H_N]
            out[H_W] = (float(raw[H_W_HI]) * TWO40 + float(raw[H_W])) * q["weight"]
            out[H_W2] = (float(raw[H_W2_HI]) * TWO40 + float(raw[H_W2])) * q["weight_sq"]
            return out

        # the clean block, out of place and in place, the sentinels behind it intact (fetch); the outside cell is converted too
        out, err = finalize(rt, torch, p, base)
        assert err is None
        np.testing.assert_array_equal(out, want_of(base))
        assert out[-CELL + A_N] == base[-CELL + A_N] > 0
        out2, err = finalize(rt, torch, p, base, in_place=True)
        assert err is None and np.array_equal(out, out2)
        a = L.split_aperture(out, nx, ny)
        assert a["outside"]["N"] == base[-CELL + A_N] and a["counts"].sum() + a["outside"]["N"] == a["head"]["N_PASSED"]
        first, outside = HEAD, HEAD + nx * ny * CELL
        # one stray quantum, one stray count: in the first cell and in the outside cell
        for cell in (first, outside):
            for slot in (A_W, A_W2, A_N):
                for d in (1, -1):
                    b = base.copy()
                    b[cell + slot] += d
                    assert b[cell + slot] >= 0
                    _, err = finalize(rt, torch, p, b)
                    assert err is not None and "do not add up" in str(err) and "negative" not in str(err), (cell, slot, d, str(err))
        # -1 and 2^62 are refused, in a cell, in the outside cell and in the head
        for slot in (first + A_N, outside + A_W, outside + A_N, H_N):
            for value in (-1, LIMIT):
                b = base.copy()
                b[slot] = value
                _, err = finalize(rt, torch, p, b)
                assert err is not None and "negative or >= 2^62" in str(err), (slot, value, str(err))
        out, err = finalize(rt, torch, p, base)                         # the clean twin still passes: no status is left behind
        assert err is None
        # squared weights that average below 2^6 quanta per passed ray: NaN in every SUM_WEIGHTS_SQ slot, no error
        b = np.zeros(base.size, dtype=np.int64)
        b[H_N], b[H_W], b[H_W2] = 256, 4096 * 256, 64 * 256 - 1
        b[first + A_N], b[first + A_W], b[first + A_W2] = 200, 4096 * 200, 64 * 200
        b[outside + A_N], b[outside + A_W], b[outside + A_W2] = 56, 4096 * 56, 64 * 56 - 1
        out, err = finalize(rt, torch, p, b)
        assert err is None
        slots = out[HEAD:].reshape(-1, CELL)
        assert np.isnan(out[H_W2]) and np.isnan(slots[:, A_W2]).all() and np.isnan(out).sum() == 1 + nx * ny + 1
        assert out[H_W] == 4096 * 256 * q["weight"] and slots[0, A_W] == 4096 * 200 * q["weight"] and slots[-1, A_N] == 56
        b[H_W2] += 1
        b[outside + A_W2] += 1
        out, err = finalize(rt, torch, p, b)
        assert err is None and not np.isnan(out).any() and out[H_W2] == 64 * 256 * q["weight_sq"]


# ---- 8: the command line ---------------------------------------------------------------------------------------
def test_cli_aperture_map_end_to_end(tmp_path):
    out = tmp_path / "a"
    r = subprocess.run([sys.executable, "-m", "solaraxionraytracing_amd", "--rays", "400000", "--outpath", str(out), "--apertureMap",
                        "--apertureBins", "64"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    total = float([l for l in r.stdout.splitlines() if l.startswith("The total flux")][0].split()[-1])
    passed = int([l for l in r.stdout.splitlines() if l.startswith("Passed axions ")][0].split()[-1])
    line = [l for l in r.stdout.splitlines() if l.startswith("--apertureMap:")][0]
    m = aperture.load_map(str(out / "aperture_map_IAXO.npz"))
    assert m["counts"].shape == m["weights"].shape == m["weights_sq"].shape == (64, 64)
    assert m["x_edges"].shape == m["y_edges"].shape == (65,) and m["n_rays"] == 400000
    assert m["x_edges"][0] == -m["x_edges"][-1] == m["y_edges"][0] < -350.0
    assert int(m["counts"].sum() + m["outside"]["N"]) == passed > 1000                       # counts sum to "Passed axions"
    assert m["weights"].sum() + m["outside"]["SUM_WEIGHTS"] == pytest.approx(total, rel=1e-9)  # the map's sum + outside = the total flux
    assert m["head"]["N_PASSED"] == passed and m["head"]["SUM_WEIGHTS"] == pytest.approx(total, rel=1e-9)
    rw = aperture.reweight(m, np.ones((64, 64)))
    assert rw["flux"] == pytest.approx(total, rel=1e-9) and rw["uncovered"] == 0.0            # the default window holds the whole pupil
    assert m["outside"] == dict(N=0.0, SUM_WEIGHTS=0.0, SUM_WEIGHTS_SQ=0.0)
    assert line.endswith("outside the window: 0 passed axions, share of the flux 0")
    rows = np.loadtxt(out / "aperture_image_IAXO.csv", delimiter=",", skiprows=1)
    assert rows.shape == (64 * 64, 5) and int(rows[:, 2].sum()) == passed
    assert rows[:, 3].sum() == pytest.approx(total, rel=1e-9)
    np.testing.assert_array_equal(rows[:, 3], m["weights"].ravel())
    prof = aperture.radial_profile(m, 50)
    assert prof["flux"].sum() == pytest.approx(total, rel=1e-9) and prof["flux"][:10].sum() == 0.0      # the bore of the optic is dark
    # with the X-ray test source, and a window that cuts the pupil: the outside share is printed
    r = subprocess.run([sys.executable, "-m", "solaraxionraytracing_amd", "--rays", "100000", "--outpath", str(tmp_path / "x"), "--apertureMap",
                        "--xrayTest", "--apertureBins", "16", "--apertureWindow", "0,352,-100,250"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    mx = aperture.load_map(str(tmp_path / "x" / "aperture_map_IAXO.npz"))
    assert mx["outside"]["N"] > 1000 and 0.3 < aperture.reweight(mx, np.ones((16, 16)))["uncovered"] < 1.0
    for extra in (["--originMap"], ["--shellBreakdown"], ["--emissionChannels", "terms"], ["--massScanMin", "0", "--massScanMax", "0.1"]):
        r = subprocess.run([sys.executable, "-m", "solaraxionraytracing_amd", "--outpath", str(tmp_path / "b"), "--apertureMap"] + extra,
                           capture_output=True, text=True, timeout=120, cwd=ROOT)
        assert r.returncode == 2 and "--apertureMap" in r.stderr, (extra, r.returncode)
        assert not (tmp_path / "b").exists()


# ---- 9: one context, back to back -------------------------------------------------------------------------------
def test_one_context_through_every_entry_back_to_back():
    import torch
    n, seed = 100_000, 31
    with Tracer(setup_of("babyiaxo_xmm")) as rt:
        rt.set_accumulation_mode("fixed64")
        grid(rt, 48, 20, BABY)
        ref = run_hist(rt, torch, n, seed)
        a1, b1 = run_aperture(rt, torch, [(0, n)], seed)
        p = params(rt, n, seed)
        acc = zeros(torch, acc_len(rt, p), torch.int64)
        sblk = zeros(torch, rt.shell_block_len(True), torch.int64)
        rt.trace_shells_device(p, acc.data_ptr(), sblk.data_ptr())
        oblk = zeros(torch, rt.origin_block_len(), torch.int64)
        acc_o = zeros(torch, acc_len(rt, p), torch.int64)
        rt.trace_origin_device(p, acc_o.data_ptr(), oblk.data_ptr())
        rt.synchronize()
        plain = run_hist(rt, torch, n, seed)
        a2, b2 = run_aperture(rt, torch, [(0, n)], seed)
    np.testing.assert_array_equal(a1, ref)
    np.testing.assert_array_equal(acc.cpu().numpy(), ref)
    np.testing.assert_array_equal(acc_o.cpu().numpy(), ref)
    np.testing.assert_array_equal(plain, ref)
    np.testing.assert_array_equal(a2, a1)
    np.testing.assert_array_equal(b2, b1)                                          # the first and the last block are equal
    head, slots = split(b1, 48, 20)
    n_passed, _, _ = assert_conserved(head, slots, scalars_of(a1))
    assert n_passed == int(oblk.cpu().numpy()[L.ORIGIN_HEAD_SLOTS["N_PASSED"]]) > 1000
