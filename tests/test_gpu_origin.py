"""Solar-origin map of the histogram trace (include/sart.h: sart_trace_histogram_origin_device) on the MI355X box.

Demanded here:
  * the accumulator of an origin launch equals sart_trace_histogram_device's for the same params and ray ids, raw int64 slot for slot
    in SART_ACCUM_FIXED64 (against the generic kernel variants, which the origin kernel is built on), spectra and flux-only included;
  * a host mirror, ray by ray and no ray left out, of every cell: N exact, the two sums the exact integer sums of the per-ray quanta
    (f64: within (EPS_DEVICE + n 2^-53) sum w, the envelope of tests/binned_records.py), every other cell 0 - the radius index from the
    ray's own uniform, the energy index from its energy; also on tables so small that dozens of lanes of a wave add to one cell;
  * conservation as Python integers: cells = head = the accumulator's scalars; the cells of one energy = the accumulator's energy bins;
  * against the channel entry on the same context, ids and seed: indicator fractions exactly, random fractions within N_PASSED quanta,
    and origin.reweight gives the same number;
  * splits and shards give the same integers; f64 and finalized FIXED64 agree; refused calls change nothing; crafted raw blocks through
    sart_finalize_origin_device; --originMap end to end."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import solaraxionraytracing_amd as sa
from solaraxionraytracing_amd import _lib as L
from solaraxionraytracing_amd import origin, tables

from tests.binned_records import EPS_DEVICE, U
from tests.conftest import SMALL, make_setup

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO40 = 2 ** L.FIXED_LIMB_BITS
LIMIT = 1 << 62
N_RADIAL = 1000
N_RAYS = 300_000
CASES = ["babyiaxo_xmm", "cast_llnl", "babyiaxo_xmm_gas", "babyiaxo_xmm_rot"]
SENT, SENTINEL = 64, 0x5A5A5A5A5A5A5A5A
HEAD, CELL = L.ORIGIN_HEAD, L.ORIGIN_CELL
O_N, O_W, O_W2 = L.ORIGIN["N"], L.ORIGIN["SUM_WEIGHTS"], L.ORIGIN["SUM_WEIGHTS_SQ"]
H_N, H_W, H_W2 = (L.ORIGIN_HEAD_SLOTS[k] for k in ("N_PASSED", "SUM_WEIGHTS", "SUM_WEIGHTS_SQ"))
H_W_HI, H_W2_HI = L.ORIGIN_HEAD_HI["SUM_WEIGHTS"], L.ORIGIN_HEAD_HI["SUM_WEIGHTS_SQ"]


def setup_of(name, **kw):
    args = dict(SMALL)
    args.update(kw)
    if name == "babyiaxo_xmm_rot":
        full = make_setup("babyiaxo_xmm", **kw)
        full.setup.telescope_turned_x_deg, full.setup.telescope_turned_y_deg = 0.01, 0.03
        return full
    if name == "cast_llnl":   # four coatings on groups of shells
        return sa.initFullSetup(L.ES_CAST, L.DK_INGRID2018, L.SK_VACUUM, L.TK_LLNL, **args)
    if name == "babyiaxo_xmm_gas":
        return sa.initFullSetup(stage=L.SK_GAS, **args)
    return make_setup(name, **kw)


class Tracer:
    """A RayTracer with SART_FORCE_GENERIC set while it is created (the origin kernel is the generic histogram kernel's twin)."""

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
    return rt.origin_params(n, seed, off, image_n=image_n, spectra=spectra, n_radial_bins=N_RADIAL, accumulate=accumulate)


def acc_len(rt, p):
    n_img = p.image_nx * p.image_ny
    return n_img + L.SART_ACC_COUNT + ((2 * p.n_radial_bins + 3 * (rt.full.energies.size + 1)) if p.spectra else 0)


def zeros(torch, n, dtype):
    """A zero-filled device buffer whose fill has FINISHED: torch fills on its own stream, the library launches on the context's
    (non-blocking) stream, and with params.accumulate it does no memset of its own - a fill that lands after the first atomics
    would wipe them."""
    t = torch.zeros(n, dtype=dtype, device="cuda")
    torch.cuda.synchronize()
    return t


def run_origin(rt, torch, pieces, seed, spectra=True, image_n=256, dtype=None):
    """Raw accumulator and origin block of one accumulation over the (lo, hi) ray-id pieces."""
    dtype = dtype or torch.int64
    p0 = params(rt, 1, seed, spectra=spectra, image_n=image_n)
    acc = zeros(torch, acc_len(rt, p0), dtype)
    blk = zeros(torch, rt.origin_block_len(), dtype)
    for lo, hi in pieces:
        p = params(rt, hi - lo, seed, lo, spectra, image_n, accumulate=True)
        rt.trace_origin_device(p, acc.data_ptr(), blk.data_ptr())
    rt.synchronize()
    return acc.cpu().numpy(), blk.cpu().numpy()


def run_hist(rt, torch, n, seed, off=0, spectra=True, image_n=256):
    p = params(rt, n, seed, off, spectra, image_n)
    acc = zeros(torch, acc_len(rt, p), torch.int64)
    rt.trace_histogram_device(p, acc.data_ptr())
    rt.synchronize()
    return acc.cpu().numpy()


def split(blk, shape):
    """(head [8], cells [n_radii][n_energies][4]) of a raw block."""
    assert blk.size == L.origin_block_len(*shape)
    return blk[:HEAD], blk[HEAD:].reshape(shape[0], shape[1], CELL)


def limbs(lo, hi):
    return int(hi) * TWO40 + int(lo)


def isum(a):
    """Exact sum of an int64 array as a Python int."""
    a = np.asarray(a).reshape(-1)
    return sum(int(v) for v in a[a != 0])


def passed_rays(rt, full, n, seed, off):
    """The passed rays of [off, off + n) with the (radius index, energy index) cell each was drawn at: the radius index is the lower
    bound of fluxRadiusCDF at the ray's third uniform (oracle/sart_oracle.c: get_random_point_from_solar_model), the energy index
    that of its energy in the table."""
    from oracle import oracle as O
    cols, counts = rt.trace_columns(n, ("ray_id", "pointdataX", "pointdataY", "weights", "energiesAx"), seed=seed, ray_id_offset=off)
    assert counts["n_passed"] == cols["ray_id"].size > 100
    rcdf, _ = rt.solar_tables()
    lib = O.load()
    u = (C.c_double * 6)()
    u2 = np.empty(cols["ray_id"].size)
    for i, rid in enumerate(cols["ray_id"]):
        lib.sart_oracle_uniforms(seed, int(rid), u)
        u2[i] = u[2]
    r_idx = np.minimum(np.searchsorted(rcdf, u2, side="left"), rcdf.size - 1)
    e_idx = np.searchsorted(full.energies, cols["energiesAx"])
    assert np.all(full.energies[e_idx] == cols["energiesAx"])   # (the energy grids start above the 0.03 keV clamp where they have mass)
    return dict(x=cols["pointdataX"].copy(), y=cols["pointdataY"].copy(), w=cols["weights"].copy(), r_idx=r_idx, e_idx=e_idx)


def scalars_of(acc, image_n=256):
    return acc[image_n * image_n:image_n * image_n + L.SART_ACC_COUNT]


def assert_conserved(head, cells, sc):
    """cells = head = the accumulator's scalars, as Python integers; limbs normalised; reserved slots 0."""
    assert 0 <= head[H_W] < TWO40 and 0 <= head[H_W2] < TWO40
    assert head[3] == 0 and head[6] == 0 and head[7] == 0 and not cells[:, :, 3].any()
    n, w, w2 = int(head[H_N]), limbs(head[H_W], head[H_W_HI]), limbs(head[H_W2], head[H_W2_HI])
    assert isum(cells[:, :, O_N]) == n == int(sc[L.ACC["N_PASSED"]])
    assert isum(cells[:, :, O_W]) == w == limbs(sc[L.ACC["SUM_WEIGHTS"]], sc[L.ACC_HI["SUM_WEIGHTS"]])
    assert isum(cells[:, :, O_W2]) == w2 == limbs(sc[L.ACC["SUM_WEIGHTS_SQ"]], sc[L.ACC_HI["SUM_WEIGHTS_SQ"]])
    return n, w, w2


def mirror_fixed(cells, rays, q):
    """Every cell of a raw FIXED64 map against the rays: exact, and 0 where no passed ray was drawn."""
    shape = cells.shape[:2]
    w_fx = np.rint(rays["w"] / q["weight"]).astype(np.int64)
    w2_fx = np.rint((rays["w"] * rays["w"]) / q["weight_sq"]).astype(np.int64)
    want = np.zeros(shape + (CELL,), dtype=np.int64)
    np.add.at(want[:, :, O_N], (rays["r_idx"], rays["e_idx"]), 1)
    np.add.at(want[:, :, O_W], (rays["r_idx"], rays["e_idx"]), w_fx)
    np.add.at(want[:, :, O_W2], (rays["r_idx"], rays["e_idx"]), w2_fx)
    assert int(want[:, :, O_W].max()) < LIMIT
    np.testing.assert_array_equal(cells, want)
    return want


# ---- 1: the accumulator ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_fixed64_accumulator_equals_the_histogram(name):
    import torch
    full = setup_of(name)
    seed = 7
    shape = (SMALL["n_radii"], SMALL["n_energies"])
    with Tracer(full) as rt:
        rt.set_accumulation_mode("fixed64")
        for spectra, image_n in ((True, 256), (False, 0)):
            ref = run_hist(rt, torch, N_RAYS, seed, 13, spectra, image_n)
            acc, blk = run_origin(rt, torch, [(13, 13 + N_RAYS)], seed, spectra, image_n)
            np.testing.assert_array_equal(acc, ref)
            head, cells = split(blk, shape)
            n, _, _ = assert_conserved(head, cells, scalars_of(acc, image_n))
            assert n > 100


# ---- 2 + 3: the mirror and the conservation laws -------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_host_mirror_ray_by_ray_and_conservation(name):
    import torch
    full = setup_of(name)
    n_r, n_e = SMALL["n_radii"], SMALL["n_energies"]
    seed, off = 19, 512
    with Tracer(full) as rt:
        rt.set_accumulation_mode("fixed64")
        acc, blk = run_origin(rt, torch, [(off, off + N_RAYS)], seed)
        q = rt.fixed_quanta()
        rays = passed_rays(rt, full, N_RAYS, seed, off)
        rt.set_accumulation_mode("f64")
        acc_f, blk_f = run_origin(rt, torch, [(off, off + N_RAYS)], seed, dtype=torch.float64)
    head, cells = split(blk, (n_r, n_e))
    n, w, w2 = assert_conserved(head, cells, scalars_of(acc))
    assert n == rays["w"].size                                    # no ray left out
    want = mirror_fixed(cells, rays, q)
    assert (want[:, :, O_N] == 0).sum() > 1000                    # thousands of cells saw no passed ray: they are 0 (asserted above)
    # sum over r of the cells at energy e = the accumulator's energy counts and energy weights, bin for bin
    en = acc[256 * 256 + L.SART_ACC_COUNT + 2 * N_RADIAL:]
    e_counts, e_weights = en[:n_e + 1], en[n_e + 1:2 * (n_e + 1)]
    np.testing.assert_array_equal(cells[:, :, O_N].sum(axis=0), e_counts[:n_e])
    np.testing.assert_array_equal(cells[:, :, O_W].sum(axis=0), e_weights[:n_e])
    assert e_counts[n_e] == 0 and e_weights[n_e] == 0
    # f64: N exact, the sums within (EPS_DEVICE + n 2^-53) sum w per cell - two instantiations of one source, and the summation term
    head_f, cells_f = split(blk_f, (n_r, n_e))
    np.testing.assert_array_equal(cells_f[:, :, O_N], want[:, :, O_N].astype(np.float64))
    sw, sw2 = np.zeros((n_r, n_e)), np.zeros((n_r, n_e))
    np.add.at(sw, (rays["r_idx"], rays["e_idx"]), rays["w"])
    np.add.at(sw2, (rays["r_idx"], rays["e_idx"]), rays["w"] * rays["w"])
    k = want[:, :, O_N].astype(np.float64)
    assert np.all(np.abs(cells_f[:, :, O_W] - sw) <= (EPS_DEVICE + 2 * k * U) * sw)
    assert np.all(np.abs(cells_f[:, :, O_W2] - sw2) <= (2 * EPS_DEVICE + 2 * (k + 1) * U) * sw2)
    assert not cells_f[:, :, 3].any() and np.all(cells_f[:, :, O_W][k == 0] == 0.0)
    sc_f = scalars_of(acc_f)
    assert head_f[H_N] == n == sc_f[L.ACC["N_PASSED"]]
    for hk, key in ((H_W, "SUM_WEIGHTS"), (H_W2, "SUM_WEIGHTS_SQ")):      # the same per-workgroup sums through two fold trees
        assert head_f[hk] == pytest.approx(sc_f[L.ACC[key]], rel=1e-12)
    assert cells_f[:, :, O_W].sum() == pytest.approx(head_f[H_W], rel=1e-12)


# ---- 4: a grid where lanes collide ------------------------------------------------------------------
@pytest.mark.parametrize("n_r,n_e", [(8, 16), (2, 4)])
@pytest.mark.parametrize("name", ["babyiaxo_xmm", "babyiaxo_xmm_rot"])
def test_tiny_grids_where_lanes_of_one_wave_share_a_cell(name, n_r, n_e):
    """The smallest tables: (8, 16) is the first guess, (2, 4) builds too (a table of two energies has one with mass: nothing to
    map).  A wave of 64 passed rays then adds dozens of lanes to one cell in one instruction."""
    import torch
    full = setup_of(name, n_radii=n_r, n_energies=n_e)
    seed, off, n = 29, 1024, 100_000
    with Tracer(full) as rt:
        rt.set_accumulation_mode("fixed64")
        acc, blk = run_origin(rt, torch, [(off, off + n)], seed)
        q = rt.fixed_quanta()
        rays = passed_rays(rt, full, n, seed, off)
    head, cells = split(blk, (n_r, n_e))
    n_passed, _, _ = assert_conserved(head, cells, scalars_of(acc))
    assert n_passed == rays["w"].size
    want = mirror_fixed(cells, rays, q)
    # the busiest cell takes more than a dozen lanes of an average wave of passed rays on the 2 x 4 table (half the draws fall into one
    # cell), more than one on the 8 x 16 table (4 % of the draws)
    share = want[:, :, O_N].max() / n_passed
    print(name, n_r, n_e, "busiest cell: %.1f lanes of 64" % (64 * share))
    assert 64 * share > (12 if n_r == 2 else 1)


# ---- 5 + 6: against the channel entry ------------------------------------------------------------
def run_channels(rt, torch, n, seed, off):
    p = rt.channels_params(n, seed, off, image_n=0, spectra=False)
    acc = zeros(torch, L.SART_ACC_COUNT, torch.int64)
    blk = zeros(torch, rt.channel_block_len(False, 0), torch.int64)
    rt.trace_channels_device(p, acc.data_ptr(), blk.data_ptr())
    rt.synchronize()
    t = rt.n_source_channels()
    return acc.cpu().numpy(), blk.cpu().numpy()[:t * L.CHAN_ROW].reshape(t, L.CHAN_ROW)


@pytest.mark.parametrize("name", ["babyiaxo_xmm", "cast_llnl"])
def test_indicator_bands_equal_the_channel_entry_exactly(name):
    import torch
    full = setup_of(name)
    total = tables.primakoff_emission_table(SMALL["n_radii"], SMALL["n_energies"])
    n_r, n_e = total.shape
    seed, off = 11, 256
    r_band = np.minimum(np.arange(n_r) * 4 // n_r, 3)            # four radius-index bands ...
    e_band = (np.arange(n_e) >= n_e // 3).astype(int)            # ... x two energy-index bands = 8 channels
    band_of = r_band[:, None] * 2 + e_band[None, :]
    rates = np.stack([total * (band_of == t) for t in range(8)])
    with Tracer(full) as rt:
        rt.set_source_channels(rates, total)
        rt.set_accumulation_mode("fixed64")
        acc_o, blk = run_origin(rt, torch, [(off, off + N_RAYS)], seed, spectra=False, image_n=0)
        acc_c, rows = run_channels(rt, torch, N_RAYS, seed, off)
    np.testing.assert_array_equal(acc_o, acc_c)
    head, cells = split(blk, (n_r, n_e))
    assert_conserved(head, cells, scalars_of(acc_o, 0))
    assert not cells[total == 0].any()
    for t in range(8):
        sel = band_of == t
        assert isum(cells[:, :, O_N][sel]) == int(rows[t][L.CHAN["N_CONTRIBUTING"]]), t
        assert isum(cells[:, :, O_W][sel]) == limbs(rows[t][L.CHAN["SUM_WEIGHTS"]], rows[t][L.CHAN_HI["SUM_WEIGHTS"]]), t
    assert int(rows[:, L.CHAN["N_CONTRIBUTING"]].sum()) == int(head[H_N]) and (rows[:, L.CHAN["N_CONTRIBUTING"]] > 0).sum() >= 4


@pytest.mark.parametrize("name", ["babyiaxo_xmm", "babyiaxo_xmm_gas"])
def test_random_fractions_agree_with_the_channel_entry_within_one_quantum_per_ray(name):
    """Per ray |rint(w / q) f - rint(w f / q)| <= 1 (half a quantum each side, f <= 1), so |sum_c D[c] f_t[c] - SUM_WEIGHTS_t| <=
    N_PASSED quanta; origin.reweight(rates_old = 1, rates_new = f_t) forms the same sum."""
    import torch
    from fractions import Fraction
    full = setup_of(name)
    n_r, n_e = SMALL["n_radii"], SMALL["n_energies"]
    rng = np.random.default_rng(1234 + 3)
    frac = rng.random((3, n_r, n_e))
    frac[rng.random(frac.shape) < 0.1] = 0.0
    seed, off = 23, 0
    with Tracer(full) as rt:
        rt.set_source_channels(frac, np.ones((n_r, n_e)))
        rt.set_accumulation_mode("fixed64")
        acc_o, blk = run_origin(rt, torch, [(off, off + N_RAYS)], seed, spectra=False, image_n=0)
        _, rows = run_channels(rt, torch, N_RAYS, seed, off)
        q = rt.fixed_quanta()
    head, cells = split(blk, (n_r, n_e))
    n_passed, _, _ = assert_conserved(head, cells, scalars_of(acc_o, 0))
    d_fx = cells[:, :, O_W]
    m = dict(counts=cells[:, :, O_N], weights=d_fx.astype(np.float64) * q["weight"], weights_sq=cells[:, :, O_W2] * q["weight_sq"])
    nz = np.nonzero(d_fx)
    for t in range(3):
        chan = limbs(rows[t][L.CHAN["SUM_WEIGHTS"]], rows[t][L.CHAN_HI["SUM_WEIGHTS"]])
        exact = sum(Fraction(int(d)) * Fraction(float(f)) for d, f in zip(d_fx[nz], frac[t][nz]))
        diff = abs(exact - chan)
        print(name, t, "sum D f - SUM_WEIGHTS_t = %.3f quanta of %d allowed" % (float(exact - chan), n_passed))
        assert diff <= n_passed, (t, float(diff), n_passed)
        assert chan > 1000 * n_passed                                     # (the bound is tight: 1e-3 of the sum at most)
        rw = origin.reweight(m, np.ones((n_r, n_e)), frac[t])
        assert rw["flux"] == pytest.approx(float(exact) * q["weight"], rel=1e-12)
        assert rw["flux"] == pytest.approx(math.fsum((m["weights"] * frac[t]).reshape(-1)), rel=1e-14)


# ---- 7: splits and modes -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["babyiaxo_xmm_gas", "babyiaxo_xmm_rot"])
def test_splits_and_shards_give_the_same_integers(name):
    import torch
    full = setup_of(name)
    n, seed = N_RAYS, 5
    shape = (SMALL["n_radii"], SMALL["n_energies"])
    with Tracer(full) as rt:
        rt.set_accumulation_mode("fixed64")
        a1, b1 = run_origin(rt, torch, [(0, n)], seed)
        a2, b2 = run_origin(rt, torch, [(0, 77_777), (77_777, n)], seed)
        a3, b3 = run_origin(rt, torch, [(0, 123_456)], seed)
        a4, b4 = run_origin(rt, torch, [(123_456, n)], seed)
    np.testing.assert_array_equal(a1, a2)
    np.testing.assert_array_equal(b1, b2)
    # shards summed as int64 (what an all-reduce of the raw buffers does); the limbs are renormalised by value, not slot for slot
    h1, c1 = split(b1, shape)
    h34, c34 = split(b3 + b4, shape)
    np.testing.assert_array_equal(c1, c34)
    assert h1[H_N] == h34[H_N]
    assert limbs(h1[H_W], h1[H_W_HI]) == limbs(h34[H_W], h34[H_W_HI]) and limbs(h1[H_W2], h1[H_W2_HI]) == limbs(h34[H_W2], h34[H_W2_HI])


@pytest.mark.parametrize("name", ["babyiaxo_xmm", "cast_llnl"])
def test_f64_and_finalized_fixed64_agree(name):
    full = setup_of(name)
    with Tracer(full) as rt:
        img_f, s_f, sp_f, o_f = rt.trace_origin(N_RAYS, seed=9)
        rt.set_accumulation_mode("fixed64")
        img_x, s_x, sp_x, o_x = rt.trace_origin(N_RAYS, seed=9)     # (its finalize checks the conservation laws on the device)
        q = rt.fixed_quanta()
    # FIXED64 rounds every ray's contribution to its quantum (<= q / 2 each): a cell of k rays agrees to k q / 2 in absolute terms
    np.testing.assert_array_equal(o_f["counts"], o_x["counts"])
    k = o_f["counts"]
    assert np.all(np.abs(o_x["weights"] - o_f["weights"]) <= 1e-11 * o_f["weights"] + 0.5 * q["weight"] * k)
    assert np.all(np.abs(o_x["weights_sq"] - o_f["weights_sq"]) <= 1e-11 * o_f["weights_sq"] + 0.5 * q["weight_sq"] * k)
    assert o_x["head"]["N_PASSED"] == o_f["head"]["N_PASSED"] == s_f["N_PASSED"] == k.sum()
    for key in ("SUM_WEIGHTS", "SUM_WEIGHTS_SQ"):
        assert o_x["head"][key] == s_x[key]                                        # the same integers, the same quantum
        assert o_f["head"][key] == pytest.approx(s_f[key], rel=1e-12)
        assert o_x["head"][key] == pytest.approx(o_f["head"][key], rel=1e-9)
    assert o_x["weights"].sum() == pytest.approx(s_x["SUM_WEIGHTS"], rel=1e-12)
    assert origin.radial_profile(o_x).sum() == pytest.approx(s_x["SUM_WEIGHTS"], rel=1e-12)
    np.testing.assert_allclose(o_x["weights"].sum(axis=0), sp_x["energy_weights"][:-1], rtol=1e-11, atol=1e-300)


# ---- 8: error paths --------------------------------------------------------------------------------------
def test_invalid_arguments_leave_the_context_unchanged():
    """After EVERY refused call: the setup bytes and a following launch are what they were, and nothing was written."""
    import torch
    full = setup_of("babyiaxo_xmm")
    n, seed = 50_000, 4
    with Tracer(full) as rt:
        lib, h = rt.lib, rt.handle
        rt.set_accumulation_mode("fixed64")
        p_good = params(rt, n, seed)
        acc = zeros(torch, acc_len(rt, p_good), torch.int64)
        blk = zeros(torch, rt.origin_block_len(), torch.int64)
        s0 = L.Setup()
        L.check(lib.sart_get_setup(h, C.byref(s0)))
        a0, b0 = run_origin(rt, torch, [(0, n)], seed)
        np.testing.assert_array_equal(a0, run_hist(rt, torch, n, seed))

        def refused(rc, code=L.SART_ERR_INVALID_ARGUMENT, *words):
            msg = lib.sart_last_error()
            assert rc == code, (rc, msg)
            for w in words:
                assert w in msg, (w, msg)
            s1 = L.Setup()
            L.check(lib.sart_get_setup(h, C.byref(s1)))
            assert bytes(s0) == bytes(s1)
            a1, b1 = run_origin(rt, torch, [(0, n)], seed)
            np.testing.assert_array_equal(a1, a0)
            np.testing.assert_array_equal(b1, b0)

        def trace_rc(p, a, b):
            return lib.sart_trace_histogram_origin_device(h, C.byref(p), C.c_void_p(a), C.c_void_p(b))

        def fin_rc(p, a, b):
            return lib.sart_finalize_origin_device(h, C.byref(p) if p is not None else None, C.c_void_p(a), C.c_void_p(b))

        refused(trace_rc(p_good, 0, blk.data_ptr()), L.SART_ERR_INVALID_ARGUMENT, b"NULL")
        refused(trace_rc(p_good, acc.data_ptr(), 0), L.SART_ERR_INVALID_ARGUMENT, b"NULL")
        refused(lib.sart_trace_histogram_origin_device(h, None, C.c_void_p(acc.data_ptr()), C.c_void_p(blk.data_ptr())))
        refused(lib.sart_trace_histogram_origin_device(None, C.byref(p_good), C.c_void_p(acc.data_ptr()), C.c_void_p(blk.data_ptr())))
        refused(fin_rc(p_good, 0, blk.data_ptr()))
        refused(fin_rc(p_good, blk.data_ptr(), 0))
        refused(fin_rc(None, blk.data_ptr(), blk.data_ptr()))
        refused(lib.sart_trace_histogram_origin(h, None, None, None, None, None))
        for field, value, word in (("image_nx", -1, b"image"), ("image_nx", 0, b"image"), ("image_x_max", -1.0, b"image"),
                                   ("n_radial_bins", 0, b"spectra"), ("radial_max", 0.0, b"spectra")):
            p = params(rt, n, seed)
            setattr(p, field, value)
            refused(trace_rc(p, acc.data_ptr(), blk.data_ptr()), L.SART_ERR_INVALID_ARGUMENT, word)
            refused(fin_rc(p, blk.data_ptr(), blk.data_ptr()), L.SART_ERR_INVALID_ARGUMENT, word)
            refused(lib.sart_trace_histogram_origin(h, C.byref(p), None, None, None, None), L.SART_ERR_INVALID_ARGUMENT, word)
        rt.synchronize()
        assert int(acc.abs().sum()) == 0 and int(blk.abs().sum()) == 0     # no refused call wrote to the caller's buffers
    # a context without solar tables: NOT_READY (the shared helper refuses a spectra request there first, as for the shells)
    lib = L.load_sart()
    h = C.c_void_p()
    L.check(lib.sart_create(0, C.byref(h)))
    try:
        L.check(lib.sart_set_setup(h, C.byref(full.setup)))
        acc = zeros(torch, L.SART_ACC_COUNT, torch.float64)
        blk = zeros(torch, L.origin_block_len(0, 0) + 64, torch.float64)
        p = L.TraceParams()
        C.memmove(C.byref(p), C.byref(p_good), C.sizeof(p))
        p.image_nx = p.image_ny = p.spectra = 0
        rc = lib.sart_trace_histogram_origin_device(h, C.byref(p), C.c_void_p(acc.data_ptr()), C.c_void_p(blk.data_ptr()))
        assert rc == L.SART_ERR_NOT_READY and b"solar tables" in lib.sart_last_error()
        rc = lib.sart_finalize_origin_device(h, C.byref(p), C.c_void_p(blk.data_ptr()), C.c_void_p(blk.data_ptr()))
        assert rc == L.SART_ERR_NOT_READY and b"solar tables" in lib.sart_last_error()
        p.spectra, p.n_radial_bins, p.radial_max = 1, 10, 10.0
        rc = lib.sart_trace_histogram_origin_device(h, C.byref(p), C.c_void_p(acc.data_ptr()), C.c_void_p(blk.data_ptr()))
        assert rc == L.SART_ERR_INVALID_ARGUMENT and b"spectra" in lib.sart_last_error()
        torch.cuda.synchronize()
        assert float(acc.abs().sum()) == 0.0 and float(blk.abs().sum()) == 0.0
    finally:
        lib.sart_destroy(h)
    # the X-ray test source has no solar draw
    with Tracer(make_setup("babyiaxo_xmm_xray")) as rt:
        lib, h = rt.lib, rt.handle
        s0 = L.Setup()
        L.check(lib.sart_get_setup(h, C.byref(s0)))
        _, sum0 = rt.trace_histogram(20_000, seed=seed)
        p = params(rt, 1000, seed)
        acc = zeros(torch, acc_len(rt, p), torch.float64)
        blk = zeros(torch, rt.origin_block_len(), torch.float64)
        with pytest.raises(L.SartError) as e:
            rt.trace_origin_device(p, acc.data_ptr(), blk.data_ptr())
        assert e.value.code == L.SART_ERR_INVALID_ARGUMENT and "test source" in str(e.value)
        with pytest.raises(L.SartError) as e:
            rt.trace_origin(1000, seed=seed)
        assert e.value.code == L.SART_ERR_INVALID_ARGUMENT and "test source" in str(e.value)
        s1 = L.Setup()
        L.check(lib.sart_get_setup(h, C.byref(s1)))
        assert bytes(s0) == bytes(s1)
        sum1 = rt.trace_histogram(20_000, seed=seed)[1]
        assert {k: v for k, v in sum1.items() if k.startswith("N_")} == {k: v for k, v in sum0.items() if k.startswith("N_")}
        assert sum1["SUM_WEIGHTS"] == pytest.approx(sum0["SUM_WEIGHTS"], rel=1e-12)     # (f64 atomics: the order of the additions)
        assert float(acc.abs().sum()) == 0.0 and float(blk.abs().sum()) == 0.0


# ---- 9: crafted raw blocks ----------------------------------------------------------------------------------
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
    rt.finalize_origin_device(p, d_raw.data_ptr(), None if in_place else d_out.data_ptr())
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


def crafted_block(rng, n_r, n_e):
    """A consistent raw block: a tenth of the cells occupied, by rays of 2^13 .. 2^45 quanta (limbs in use), the head their sums."""
    cells = np.zeros((n_r, n_e, CELL), dtype=np.int64)
    occ = rng.random((n_r, n_e)) < 0.1
    occ[0, 0] = occ[n_r - 1, n_e - 1] = occ[n_r // 2, 255 % n_e] = True
    k = int(occ.sum())
    cells[:, :, O_N][occ] = rng.integers(1, 1000, k)
    cells[:, :, O_W][occ] = cells[:, :, O_N][occ] * rng.integers(1 << 13, 1 << 35, k)
    cells[:, :, O_W2][occ] = cells[:, :, O_N][occ] * rng.integers(1 << 7, 1 << 33, k)
    head = np.zeros(HEAD, dtype=np.int64)
    w, w2 = isum(cells[:, :, O_W]), isum(cells[:, :, O_W2])
    head[H_N] = isum(cells[:, :, O_N])
    head[H_W], head[H_W_HI] = w % TWO40, w // TWO40
    head[H_W2], head[H_W2_HI] = w2 % TWO40, w2 // TWO40
    assert head[H_W_HI] > 0 and head[H_W2_HI] > 0
    return np.concatenate([head, cells.reshape(-1)])


def test_finalize_on_crafted_blocks():
    import torch
    n_r, n_e = SMALL["n_radii"], SMALL["n_energies"]
    with Tracer(setup_of("babyiaxo_xmm")) as rt:
        rt.set_accumulation_mode("fixed64")
        acc = zeros(torch, L.SART_ACC_COUNT, torch.int64)
        rt.trace_histogram_device(rt.trace_params(1000, seed=3, image_n=0), acc.data_ptr())    # freezes the quanta
        rt.synchronize()
        q = rt.fixed_quanta()
        p = params(rt, 1, 3, spectra=False, image_n=0)
        rng = np.random.default_rng(41)
        base = crafted_block(rng, n_r, n_e)
        n_slots = base.size
        assert n_slots == rt.origin_block_len()

        def want_of(raw):
            out = np.zeros(raw.size)
            c = raw[HEAD:].reshape(-1, CELL)
            o = out[HEAD:].reshape(-1, CELL)
            o[:, O_N] = c[:, O_N]
            o[:, O_W] = c[:, O_W].astype(np.float64) * q["weight"]
            o[:, O_W2] = c[:, O_W2].astype(np.float64) * q["weight_sq"]
            out[H_N] = raw[H_N]
            out[H_W] = (float(raw[H_W_HI]) * TWO40 + float(raw[H_W])) * q["weight"]
            out[H_W2] = (float(raw[H_W2_HI]) * TWO40 + float(raw[H_W2])) * q["weight_sq"]
            return out

        # the clean block, out of place and in place; and with unnormalised limbs (a sum over ranks)
        out, err = finalize(rt, torch, p, base)
        assert err is None
        np.testing.assert_array_equal(out, want_of(base))
        out2, err = finalize(rt, torch, p, base, in_place=True)
        assert err is None and np.array_equal(out, out2)
        unn = base.copy()
        unn[H_W] += 3 * TWO40
        unn[H_W_HI] -= 3
        out3, err = finalize(rt, torch, p, unn)
        assert err is None and np.array_equal(out3, out)
        first, mid, last = HEAD, HEAD + ((n_r // 2) * n_e + 255) * CELL, HEAD + (n_r * n_e - 1) * CELL
        # one stray quantum, one stray count: in the first, a middle and the last cell, and in the head
        for cell in (first, mid, last):
            for slot, word in ((O_W, "do not add up"), (O_W2, "do not add up"), (O_N, "do not add up")):
                for d in (1, -1):
                    a = base.copy()
                    a[cell + slot] += d
                    assert a[cell + slot] >= 0
                    _, err = finalize(rt, torch, p, a)
                    assert err is not None and word in str(err) and "negative" not in str(err), (cell, slot, d, str(err))
        for slot in (H_N, H_W, H_W_HI, H_W2, H_W2_HI):
            a = base.copy()
            a[slot] += 1
            _, err = finalize(rt, torch, p, a)
            assert err is not None and "do not add up" in str(err), slot
        # a negative slot, a slot at 2^62; 2^62 - 1 is in range (the sums no longer agree, but nothing wrapped)
        # (a reserved slot is in no sum: in range it is no error at all)
        for slot, summed in ((first + O_N, True), (first + O_W, True), (mid + O_W2, True), (last + O_W, True), (last + 3, False),
                             (H_N, True), (H_W_HI, True), (3, False), (7, False)):
            for value, wrapped in ((-1, True), (LIMIT, True), (LIMIT - 1, False)):
                a = base.copy()
                a[slot] = value
                _, err = finalize(rt, torch, p, a)
                assert (err is not None) == (wrapped or summed), (slot, value, str(err))
                assert ("negative or >= 2^62" in str(err)) == wrapped, (slot, value, str(err))
        out, err = finalize(rt, torch, p, base)                         # the clean twin still passes: no status is left behind
        assert err is None
        # squared weights that average below 2^6 quanta per passed ray: NaN in every SUM_WEIGHTS_SQ slot, no error
        a = np.zeros(n_slots, dtype=np.int64)
        a[H_N], a[H_W], a[H_W2] = 256, 4096 * 256, 64 * 256 - 1
        a[first + O_N], a[first + O_W], a[first + O_W2] = 200, 4096 * 200, 64 * 200
        a[last + O_N], a[last + O_W], a[last + O_W2] = 56, 4096 * 56, 64 * 56 - 1
        out, err = finalize(rt, torch, p, a)
        assert err is None
        cells = out[HEAD:].reshape(-1, CELL)
        assert np.isnan(out[H_W2]) and np.isnan(cells[:, O_W2]).all() and np.isnan(out).sum() == 1 + n_r * n_e
        assert out[H_W] == 4096 * 256 * q["weight"] and cells[0, O_W] == 4096 * 200 * q["weight"] and cells[-1, O_N] == 56
        a[H_W2] += 1
        a[last + O_W2] += 1
        out, err = finalize(rt, torch, p, a)
        assert err is None and not np.isnan(out).any() and out[H_W2] == 64 * 256 * q["weight_sq"]
        # fewer than 256 rays are not judged
        a[H_N], a[first + O_N], a[H_W2], a[first + O_W2] = 255, 199, 1, 0
        a[last + O_W2] = 1
        out, err = finalize(rt, torch, p, a)
        assert err is None and not np.isnan(out).any()


# ---- 10: the command line ---------------------------------------------------------------------------------------
def test_cli_origin_map_end_to_end(tmp_path):
    out = tmp_path / "a"
    r = subprocess.run([sys.executable, "-m", "solaraxionraytracing_amd", "--rays", "400000", "--outpath", str(out), "--originMap"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    total = float([l for l in r.stdout.splitlines() if l.startswith("The total flux")][0].split()[-1])
    passed = int([l for l in r.stdout.splitlines() if l.startswith("Passed axions ")][0].split()[-1])
    m = origin.load_map(str(out / "origin_map_IAXO.npz"))
    shape = (tables.N_RADII, tables.N_ENERGIES)
    assert m["counts"].shape == m["weights"].shape == m["weights_sq"].shape == m["rates"].shape == shape
    assert m["radii"].shape == (shape[0],) and m["energies"].shape == (shape[1],) and float(m["n_rays"]) == 400000
    assert int(m["counts"].sum()) == passed > 1000
    img = np.loadtxt(out / "axion_image_IAXO.csv", delimiter=",", skiprows=1, usecols=2)
    assert img.sum() == pytest.approx(total, rel=1e-9)
    assert m["weights"].sum() == pytest.approx(total, rel=1e-9)            # sum of the map = the flux of the run
    prof = np.loadtxt(out / "flux_by_solar_radius_IAXO.csv", delimiter=",", skiprows=1)
    assert prof.shape == (shape[0], 6)
    np.testing.assert_allclose(prof[:, 3], origin.radial_profile(m), rtol=1e-15)
    assert prof[:, 3].sum() == pytest.approx(m["weights"].sum(), rel=1e-12) and prof[:, 5].sum() == pytest.approx(1.0, rel=1e-12)
    assert int(prof[:, 2].sum()) == passed
    same = origin.reweight(m, m["rates"], m["rates"])
    assert same["flux"] == pytest.approx(m["weights"].sum(), rel=1e-12) and same["uncovered"] == 0.0
    for extra in (["--xrayTest"], ["--shellBreakdown"], ["--emissionChannels", "terms"], ["--massScanMin", "0", "--massScanMax", "0.1"]):
        r = subprocess.run([sys.executable, "-m", "solaraxionraytracing_amd", "--outpath", str(tmp_path / "b"), "--originMap"] + extra,
                           capture_output=True, text=True, timeout=120, cwd=ROOT)
        assert r.returncode == 2 and "--originMap" in r.stderr, (extra, r.returncode)
        assert not (tmp_path / "b").exists()
