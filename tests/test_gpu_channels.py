"""Emission-channel breakdown of the histogram trace (include/sart.h: sart_trace_histogram_channels_device) on the MI355X box.

Demanded here:
  * the accumulator of a channels launch equals sart_trace_histogram_device's for the same params and ray ids, raw int64 slot for slot
    in SART_ACCUM_FIXED64 (against the generic kernel variants, which the channel kernel is built on; the counters also against the
    specialised ones);
  * indicator channels (every fraction 0 or 1, a partition of the (radius, energy) grid): the sums over channels are the global sums,
    image and energy spectrum, exactly as integers, and a channel's energy bins are the global ones inside its band;
  * a host mirror, ray by ray, of every row, energy bin, pixel and OUTSIDE slot for random fraction tables of 1, 3 and 8 channels
    (strides 1, 4 and 8): the radius index from the ray's own uniform, the energy index from its energy;
  * per channel, pixels + outside = energy bins = SUM_WEIGHTS as integers;
  * the real emission components: sums across channels within N_PASSED (T + 1) / 2 quanta;
  * the two set forms give the same bits, the getter is numpy's rates / total; splits and shards give the same integers; f64 and
    finalized FIXED64 agree; invalid arguments change nothing; --emissionChannels end to end."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import solaraxionraytracing_amd as sa
from solaraxionraytracing_amd import _lib as L
from solaraxionraytracing_amd import raytracer as R
from solaraxionraytracing_amd import tables

from tests.conftest import SMALL, make_setup

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO40 = 2 ** L.FIXED_LIMB_BITS
N_RADIAL = 1000
N_RAYS = 300_000
CASES = ["babyiaxo_xmm", "cast_llnl", "babyiaxo_xmm_gas", "babyiaxo_xmm_rot"]


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


_TOTAL = {}


def total_table():
    """The emission table the SMALL setups' CDFs are made from (E1: Primakoff on the AGSS09 model)."""
    if "t" not in _TOTAL:
        _TOTAL["t"] = tables.primakoff_emission_table(SMALL["n_radii"], SMALL["n_energies"])
        _TOTAL["t"].setflags(write=False)
    return _TOTAL["t"]


def random_fractions(t, seed=1234):
    rng = np.random.default_rng(seed + t)
    f = rng.random((t, SMALL["n_radii"], SMALL["n_energies"]))
    f[rng.random(f.shape) < 0.1] = 0.0   # some exact zeros: no atomics, not contributing
    return f


class Tracer:
    """A RayTracer with SART_FORCE_GENERIC set while it is created (the channel kernel is the generic histogram kernel's twin)."""

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
    return rt.channels_params(n, seed, off, image_n=image_n, spectra=spectra, n_radial_bins=N_RADIAL, accumulate=accumulate)


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


def run_channels(rt, torch, pieces, seed, spectra=True, image_n=256, dtype=None):
    """Raw accumulator and channel block of one accumulation over the (lo, hi) ray-id pieces."""
    dtype = dtype or torch.int64
    p0 = params(rt, 1, seed, spectra=spectra, image_n=image_n)
    acc = zeros(torch, acc_len(rt, p0), dtype)
    blk = zeros(torch, rt.channel_block_len(spectra, image_n), dtype)
    for lo, hi in pieces:
        p = params(rt, hi - lo, seed, lo, spectra, image_n, accumulate=True)
        rt.trace_channels_device(p, acc.data_ptr(), blk.data_ptr())
    rt.synchronize()
    return acc.cpu().numpy(), blk.cpu().numpy()


def run_hist(rt, torch, n, seed, off=0, spectra=True, image_n=256):
    p = params(rt, n, seed, off, spectra, image_n)
    acc = zeros(torch, acc_len(rt, p), torch.int64)
    rt.trace_histogram_device(p, acc.data_ptr())
    rt.synchronize()
    return acc.cpu().numpy()


def split(blk, t, ne, spectra=True, image_n=256):
    """(rows [T][8], energy_weights [T][ne + 1] or None, images [T][ny][nx] or None) of a raw block."""
    assert blk.size == L.channel_block_len(t, ne, spectra, image_n, image_n)
    rows = blk[:t * L.CHAN_ROW].reshape(t, L.CHAN_ROW)
    o = t * L.CHAN_ROW
    en = None
    if spectra:
        en = blk[o:o + t * (ne + 1)].reshape(t, ne + 1)
        o += t * (ne + 1)
    img = blk[o:].reshape(t, image_n, image_n) if image_n else None
    return rows, en, img


def limbs(lo, hi):
    return int(hi) * TWO40 + int(lo)


def row_value(row, key):
    return limbs(row[L.CHAN[key]], row[L.CHAN_HI[key]])


def isum(a):
    """Exact sum of an int64 array as a Python int."""
    return sum(int(v) for v in np.asarray(a).reshape(-1)[np.asarray(a).reshape(-1) != 0])


def assert_conserved(rows, en, img):
    """Per channel, exactly: pixels + outside = energy bins = SUM_WEIGHTS; low limbs normalised; slot 6 unused."""
    for t, row in enumerate(rows):
        sw = row_value(row, "SUM_WEIGHTS")
        assert 0 <= row[L.CHAN["SUM_WEIGHTS"]] < TWO40 and 0 <= row[L.CHAN["SUM_WEIGHTS_SQ"]] < TWO40
        assert row[L.CHAN_RESERVED] == 0
        if en is not None:
            assert isum(en[t]) == sw, t
        pix = isum(img[t]) if img is not None else 0
        assert pix + row_value(row, "SUM_WEIGHTS_OUTSIDE") == sw, t


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
    assert np.all(full.energies[e_idx] == cols["energiesAx"])   # (the SMALL energy grid starts above the 0.03 keV clamp)
    return dict(x=cols["pointdataX"].copy(), y=cols["pointdataY"].copy(), w=cols["weights"].copy(), r_idx=r_idx, e_idx=e_idx)


def pixels_of(p, x, y):
    """prepareHeatmap's binning as the kernels evaluate it: (pixel index, inside)."""
    inv_x = 1.0 / ((p.image_x_max - p.image_x_min) / float(p.image_nx))
    inv_y = 1.0 / ((p.image_y_max - p.image_y_min) / float(p.image_ny))
    fx, fy = (x - p.image_x_min) * inv_x, (y - p.image_y_min) * inv_y
    inside = (fx >= 0.0) & (fx < p.image_nx) & (fy >= 0.0) & (fy < p.image_ny)
    ix, iy = np.where(inside, fx, 0.0).astype(np.int64), np.where(inside, fy, 0.0).astype(np.int64)
    return iy * p.image_nx + ix, inside


@pytest.mark.parametrize("name", CASES)
def test_fixed64_accumulator_equals_the_histogram(name):
    import torch
    full = setup_of(name)
    seed = 7
    with Tracer(full) as rt:
        rt.set_source_channels(random_fractions(3), np.ones(total_table().shape))
        rt.set_accumulation_mode("fixed64")
        for spectra, image_n in ((True, 256), (False, 0)):
            ref = run_hist(rt, torch, N_RAYS, seed, 13, spectra, image_n)
            acc, blk = run_channels(rt, torch, [(13, 13 + N_RAYS)], seed, spectra, image_n)
            np.testing.assert_array_equal(acc, ref)
            assert acc[image_n * image_n + L.ACC["N_PASSED"]] > 100
            rows, en, img = split(blk, 3, full.energies.size, spectra, image_n)
            assert_conserved(rows, en, img)
            if not image_n:   # a flux-only launch has no image: every ray is outside it
                for row in rows:
                    assert row_value(row, "SUM_WEIGHTS_OUTSIDE") == row_value(row, "SUM_WEIGHTS") > 0


@pytest.mark.parametrize("name", CASES)
def test_counters_equal_the_specialised_histogram(name):
    """Against the solar-source specialisations (no SART_FORCE_GENERIC): the same rays, so the same counters."""
    full = setup_of(name)
    with Tracer(full, generic=False) as rt:
        rt.set_source_channels(random_fractions(3), np.ones(total_table().shape))
        _, s_h = rt.trace_histogram(N_RAYS, seed=3, ray_id_offset=1)
        _, s_c, _, ch = rt.trace_channels(N_RAYS, seed=3, ray_id_offset=1)
    for k in ("N_RAYS", "N_REACHED_TELESCOPE", "N_SHELL_SELECTED", "N_HIT_NICKEL", "N_PASSED_TILL_WINDOW", "N_PASSED", "N_OUTSIDE_IMAGE"):
        assert s_h[k] == s_c[k], k
    assert s_c["SUM_WEIGHTS"] == pytest.approx(s_h["SUM_WEIGHTS"], rel=1e-12)
    assert np.all(ch["N_CONTRIBUTING"] <= s_c["N_PASSED"]) and np.all(ch["N_CONTRIBUTING"] > 0.8 * s_c["N_PASSED"])


@pytest.mark.parametrize("name", CASES)
def test_indicator_channels_partition_the_result_exactly(name):
    import torch
    full = setup_of(name)
    total = total_table()
    n_r, n_e = total.shape
    seed, off = 11, 256
    r_band = np.minimum(np.arange(n_r) * 3 // n_r, 2)     # three radius-index bands ...
    e_band = (np.arange(n_e) >= n_e // 3).astype(int)     # ... x two energy-index bands = 6 channels: stride 8
    chan_of = r_band[:, None] * 2 + e_band[None, :]
    rates = np.stack([total * (chan_of == t) for t in range(6)])
    with Tracer(full) as rt:
        rt.set_source_channels(rates, total)
        frac = rt.source_channels()
        rt.set_accumulation_mode("fixed64")
        acc, blk = run_channels(rt, torch, [(off, off + N_RAYS)], seed)
        rays = passed_rays(rt, full, N_RAYS, seed, off)
    assert set(np.unique(frac)) == {0.0, 1.0}
    np.testing.assert_array_equal(frac.sum(axis=0), (total != 0).astype(float))
    assert (total == 0).sum() > 0                                     # the small Primakoff table has cells without CDF mass ...
    assert np.all(total[rays["r_idx"], rays["e_idx"]] != 0.0)         # ... and no passed ray was drawn there
    n_img = 256 * 256
    sc = acc[n_img:n_img + L.SART_ACC_COUNT]
    rows, en, img = split(blk, 6, n_e)
    assert_conserved(rows, en, img)
    assert sc[L.ACC["N_PASSED"]] == rays["w"].size
    for key in ("SUM_WEIGHTS", "SUM_WEIGHTS_SQ"):
        assert sum(row_value(r, key) for r in rows) == limbs(sc[L.ACC[key]], sc[L.ACC_HI[key]]), key
    assert int(rows[:, L.CHAN["N_CONTRIBUTING"]].sum()) == int(sc[L.ACC["N_PASSED"]])
    np.testing.assert_array_equal(img.sum(axis=0).reshape(-1), acc[:n_img])
    g_en = acc[n_img + L.SART_ACC_COUNT + 2 * N_RADIAL:][n_e + 1:2 * (n_e + 1)]      # the accumulator's energy weights
    np.testing.assert_array_equal(en.sum(axis=0), g_en)
    assert g_en[n_e] == 0
    for t in range(6):     # a channel's energy bins: the global ones inside its energy band - for the rays of its radius band
        band = np.append(e_band == t % 2, False)
        assert np.all(en[t][~band] == 0)
    for eb in range(2):    # the three radius bands of one energy band add up to the global bins of that band
        band = np.append(e_band == eb, False)
        np.testing.assert_array_equal(sum(en[2 * rb + eb] for rb in range(3))[band], g_en[band])
    # and ray by ray: the contributing rays of a channel are those drawn in its cells
    np.testing.assert_array_equal(rows[:, L.CHAN["N_CONTRIBUTING"]], np.bincount(chan_of[rays["r_idx"], rays["e_idx"]], minlength=6))


@pytest.mark.parametrize("name,t", [("babyiaxo_xmm", 1), ("cast_llnl", 3), ("babyiaxo_xmm_gas", 8), ("babyiaxo_xmm_rot", 8)])
def test_host_mirror_ray_by_ray(name, t):
    import torch
    full = setup_of(name)
    n_e = full.energies.size
    seed, off = 19, 512
    with Tracer(full) as rt:
        rt.set_source_channels(random_fractions(t), np.ones(total_table().shape))
        frac = rt.source_channels()
        rt.set_accumulation_mode("fixed64")
        acc, blk = run_channels(rt, torch, [(off, off + N_RAYS)], seed)
        q = rt.fixed_quanta()
        rays = passed_rays(rt, full, N_RAYS, seed, off)
        p = params(rt, N_RAYS, seed, off)
    np.testing.assert_array_equal(frac, random_fractions(t))     # total = 1: the division leaves the table as it is
    rows, en, img = split(blk, t, n_e)
    assert_conserved(rows, en, img)
    pix, inside = pixels_of(p, rays["x"], rays["y"])
    assert acc[256 * 256 + L.ACC["N_OUTSIDE_IMAGE"]] == int((~inside).sum())
    for k in range(t):
        f = frac[k][rays["r_idx"], rays["e_idx"]]
        c = rays["w"] * f                                        # ONE product, then to_fixed: round to nearest even of c 2^k
        c_fx = np.rint(c / q["weight"]).astype(np.int64)
        c2_fx = np.rint((c * c) / q["weight_sq"]).astype(np.int64)
        assert row_value(rows[k], "SUM_WEIGHTS") == isum(c_fx), k
        assert row_value(rows[k], "SUM_WEIGHTS_SQ") == isum(c2_fx), k
        assert row_value(rows[k], "SUM_WEIGHTS_OUTSIDE") == isum(c_fx[~inside]), k
        assert rows[k][L.CHAN["N_CONTRIBUTING"]] == int((f > 0.0).sum()), k
        want_en = np.zeros(n_e + 1, dtype=np.int64)
        np.add.at(want_en, rays["e_idx"], c_fx)
        np.testing.assert_array_equal(en[k], want_en)
        want_img = np.zeros(256 * 256, dtype=np.int64)
        np.add.at(want_img, pix[inside], c_fx[inside])
        np.testing.assert_array_equal(img[k].reshape(-1), want_img)


def test_real_components_terms_and_couplings():
    import torch
    full = setup_of("babyiaxo_xmm", emission="agss09")
    seed = 23
    with Tracer(full) as rt:
        rt.set_accumulation_mode("fixed64")
        out = {}
        for grouping, t in (("terms", 8), ("couplings", 3)):
            names = rt.set_emission_channels(grouping)
            assert len(names) == t == rt.n_source_channels()
            acc, blk = run_channels(rt, torch, [(0, N_RAYS)], seed)
            rows, en, img = split(blk, t, full.energies.size)
            assert_conserved(rows, en, img)
            sc = acc[256 * 256:256 * 256 + L.SART_ACC_COUNT]
            n_passed = int(sc[L.ACC["N_PASSED"]])
            glob = limbs(sc[L.ACC["SUM_WEIGHTS"]], sc[L.ACC_HI["SUM_WEIGHTS"]])
            chan = [row_value(r, "SUM_WEIGHTS") for r in rows]
            # sum_t c_t rounds T times where the global sum rounds once
            bound = n_passed * (t + 1) / 2
            assert n_passed > 1000 and abs(sum(chan) - glob) <= bound, (grouping, sum(chan) - glob, bound)
            out[grouping] = (chan, n_passed, glob)
            if grouping == "couplings":
                _, s, _, ch = rt.trace_channels(N_RAYS, seed=seed)
                q = rt.fixed_quanta()["weight"]
                sig = R.coupling_signal(ch)
                assert ch["names"] == ch["couplings"] == list(R.COUPLINGS)
                assert abs(sig["flux"] - s["SUM_WEIGHTS"]) <= bound * q * (1 + 1e-12)
                assert sig["flux_error"] >= np.sqrt(s["SUM_WEIGHTS_SQ"]) * (1 - 1e-9)
                np.testing.assert_allclose(sig["image"].sum() + ch["SUM_WEIGHTS_OUTSIDE"].sum(), sig["flux"], rtol=1e-12)
    terms, n_passed, glob = out["terms"]
    assert out["couplings"][1] == n_passed and out["couplings"][2] == glob        # the same rays
    for k, coupling in enumerate(R.COUPLINGS):
        members = [terms[j] for j, term in enumerate(L.EM_TERMS) if R.TERM_COUPLING[term] == coupling]
        # the group's fraction is the rounded sum of its terms' rates over the total; each member rounds once per ray
        bound = n_passed * (len(members) + 1) / 2
        assert abs(sum(members) - out["couplings"][0][k]) <= bound, (coupling, sum(members) - out["couplings"][0][k], bound)
    assert out["couplings"][0][0] > 0 and out["couplings"][0][1] > 0     # both the g_ae and the g_agamma group carry flux


def test_host_and_device_set_forms_and_the_getter():
    import torch
    full = setup_of("babyiaxo_xmm")
    total = total_table()
    rng = np.random.default_rng(77)
    for t in (1, 2, 5, 8):
        rates = total[None, :, :] * rng.random((t,) + total.shape) / t
        with Tracer(full) as rt:
            rt.set_source_channels(rates, total)
            assert rt.n_source_channels() == t
            f_host = rt.source_channels()
            rt.clear_source_channels()
            with pytest.raises(L.SartError) as e:
                rt.source_channels()
            assert e.value.code == L.SART_ERR_NOT_READY
            d_rates, d_total = torch.from_numpy(rates).cuda(), torch.from_numpy(total.copy()).cuda()
            torch.cuda.synchronize()     # the copies run on torch's stream, the library's kernel on the context's
            rt.set_source_channels_device(d_rates.data_ptr(), d_total.data_ptr(), t, total.shape[0], total.shape[1])
            f_dev = rt.source_channels()
        with np.errstate(divide="ignore", invalid="ignore"):
            want = np.where(total[None] != 0, rates / total[None], 0.0)
        assert (total == 0).sum() > 0
        np.testing.assert_array_equal(f_host.view(np.uint64), f_dev.view(np.uint64))
        np.testing.assert_array_equal(f_host.view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("name", ["babyiaxo_xmm_gas", "babyiaxo_xmm_rot"])
def test_splits_and_shards_give_the_same_integers(name):
    import torch
    full = setup_of(name)
    n, seed, t = N_RAYS, 5, 3
    with Tracer(full) as rt:
        rt.set_source_channels(random_fractions(t), np.ones(total_table().shape))
        rt.set_accumulation_mode("fixed64")
        a1, b1 = run_channels(rt, torch, [(0, n)], seed)
        a2, b2 = run_channels(rt, torch, [(0, 77_777), (77_777, n)], seed)
        a3, b3 = run_channels(rt, torch, [(0, 123_456)], seed)
        a4, b4 = run_channels(rt, torch, [(123_456, n)], seed)
    np.testing.assert_array_equal(a1, a2)
    np.testing.assert_array_equal(b1, b2)
    # shards summed as int64 (what an all-reduce of the raw buffers does); the limbs are renormalised by value, not slot for slot
    ne = full.energies.size
    rows1, en1, img1 = split(b1, t, ne)
    rows34, en34, img34 = split(b3 + b4, t, ne)
    np.testing.assert_array_equal(en1, en34)
    np.testing.assert_array_equal(img1, img34)
    np.testing.assert_array_equal(rows1[:, L.CHAN["N_CONTRIBUTING"]], rows34[:, L.CHAN["N_CONTRIBUTING"]])
    for key in L.CHAN_HI:
        for r1, r2 in zip(rows1, rows34):
            assert row_value(r1, key) == row_value(r2, key)


@pytest.mark.parametrize("name", ["babyiaxo_xmm", "cast_llnl"])
def test_f64_and_finalized_fixed64_agree(name):
    full = setup_of(name)
    with Tracer(full) as rt:
        rt.set_source_channels(random_fractions(3), np.ones(total_table().shape))
        img_f, s_f, sp_f, ch_f = rt.trace_channels(N_RAYS, seed=9)
        rt.set_accumulation_mode("fixed64")
        img_x, s_x, sp_x, ch_x = rt.trace_channels(N_RAYS, seed=9)     # (its finalize checks the conservation laws on the device)
        q = rt.fixed_quanta()["weight"]
    # FIXED64 rounds every ray's contribution to its quantum (<= q / 2 each): a bin of k rays agrees to k q / 2 in absolute terms
    np.testing.assert_array_equal(ch_f["N_CONTRIBUTING"], ch_x["N_CONTRIBUTING"])
    for key in ("SUM_WEIGHTS", "SUM_WEIGHTS_SQ", "SUM_WEIGHTS_OUTSIDE"):
        np.testing.assert_allclose(ch_x[key], ch_f[key], rtol=1e-11, atol=1e-12 * ch_f["SUM_WEIGHTS" if key != "SUM_WEIGHTS_SQ" else key].max())
    k_max = sp_f["energy_counts"].max()
    np.testing.assert_allclose(ch_x["energy_weights"], ch_f["energy_weights"], rtol=1e-11, atol=0.5 * q * k_max)
    np.testing.assert_allclose(ch_x["images"], ch_f["images"], rtol=1e-11, atol=0.5 * q * s_f["N_PASSED"])
    assert s_x["SUM_WEIGHTS"] == pytest.approx(s_f["SUM_WEIGHTS"], rel=1e-12)
    np.testing.assert_allclose(ch_f["images"].sum(axis=(1, 2)) + ch_f["SUM_WEIGHTS_OUTSIDE"], ch_f["SUM_WEIGHTS"], rtol=1e-12)
    np.testing.assert_allclose(ch_f["energy_weights"].sum(axis=1), ch_f["SUM_WEIGHTS"], rtol=1e-12)


def test_invalid_arguments_leave_the_context_unchanged():
    """After EVERY refused call: the setup bytes, the fractions and a following launch are what they were."""
    import torch
    full = setup_of("babyiaxo_xmm")
    total = total_table()
    n_r, n_e = total.shape
    good_rates = random_fractions(3)
    ones = np.ones(total.shape)
    n, seed = 50_000, 4
    with Tracer(full) as rt:
        lib, h = rt.lib, rt.handle
        rt.set_accumulation_mode("fixed64")
        p_good = params(rt, n, seed)
        acc = zeros(torch, acc_len(rt, p_good), torch.int64)
        blk = zeros(torch, L.channel_block_len(3, n_e, True, 256, 256), torch.int64)
        s0 = L.Setup()
        L.check(lib.sart_get_setup(h, C.byref(s0)))
        h0 = run_hist(rt, torch, n, seed)
        state = {}

        def unchanged():
            s1 = L.Setup()
            L.check(lib.sart_get_setup(h, C.byref(s1)))
            assert bytes(s0) == bytes(s1)
            if state:
                np.testing.assert_array_equal(rt.source_channels(), state["f0"])
                a1, b1 = run_channels(rt, torch, [(0, n)], seed)
                np.testing.assert_array_equal(a1, state["a0"])
                np.testing.assert_array_equal(b1, state["b0"])
            else:
                assert lib.sart_get_source_channels(h, None, None) == L.SART_ERR_NOT_READY
                np.testing.assert_array_equal(run_hist(rt, torch, n, seed), h0)

        def refused(rc, code=L.SART_ERR_INVALID_ARGUMENT, *words):
            msg = lib.sart_last_error()
            assert rc == code, (rc, msg)
            for w in words:
                assert w in msg, (w, msg)
            unchanged()

        def trace_rc(p, a, b):
            return lib.sart_trace_histogram_channels_device(h, C.byref(p), C.c_void_p(a), C.c_void_p(b))

        def set_rc(rates, tot, t, nr, ne):
            return lib.sart_set_source_channels(h, L.as_dp(rates) if rates is not None else None, L.as_dp(tot) if tot is not None else None, t, nr, ne)

        # no channels yet
        refused(trace_rc(p_good, acc.data_ptr(), blk.data_ptr()), L.SART_ERR_NOT_READY)
        refused(lib.sart_finalize_channels_device(h, C.byref(p_good), C.c_void_p(blk.data_ptr()), C.c_void_p(blk.data_ptr())), L.SART_ERR_NOT_READY)
        rt.set_source_channels(good_rates, ones)
        state["f0"] = rt.source_channels()
        state["a0"], state["b0"] = run_channels(rt, torch, [(0, n)], seed)
        np.testing.assert_array_equal(state["a0"], h0)
        refused(set_rc(good_rates, ones, 3, n_r - 1, n_e))                                       # wrong table shape
        refused(set_rc(good_rates, ones, 3, n_r, n_e + 1))
        refused(set_rc(good_rates, ones, 0, n_r, n_e))                                           # T = 0 and T = 9
        refused(set_rc(np.zeros((9, n_r, n_e)), ones, 9, n_r, n_e))
        refused(set_rc(None, ones, 3, n_r, n_e))                                                 # NULL pointers
        refused(set_rc(good_rates, None, 3, n_r, n_e))
        refused(lib.sart_set_source_channels_device(h, None, None, 3, n_r, n_e))
        bad = good_rates.copy()
        bad[1, 17, 5] = -1e-3                                                                    # a negative rate
        refused(set_rc(bad, ones, 3, n_r, n_e), L.SART_ERR_INVALID_ARGUMENT, b"channel 1", b"radius index 17, energy index 5")
        bad = good_rates.copy()
        bad[2, 399, 299] = np.nan
        refused(set_rc(bad, ones, 3, n_r, n_e), L.SART_ERR_INVALID_ARGUMENT, b"channel 2", b"radius index 399, energy index 299")
        bad_total = ones.copy()
        bad_total[7, 7] = -1.0
        refused(set_rc(good_rates, bad_total, 3, n_r, n_e), L.SART_ERR_INVALID_ARGUMENT, b"total_rates", b"radius index 7, energy index 7")
        bad = good_rates.copy()
        bad[2, 123, 45] = 1.0 + 2.0 ** -40                                                       # a rate above the total: the FIRST cell is named
        bad[2, 200, 7] = 2.0
        refused(set_rc(bad, ones, 3, n_r, n_e), L.SART_ERR_INVALID_ARGUMENT, b"channel 2", b"radius index 123, energy index 45", b"exceeds the total")
        # trace: NULL pointers, bad image / spectra params
        refused(trace_rc(p_good, 0, blk.data_ptr()))
        refused(trace_rc(p_good, acc.data_ptr(), 0))
        refused(lib.sart_finalize_channels_device(h, C.byref(p_good), None, C.c_void_p(blk.data_ptr())))
        for field, value in (("image_nx", -1), ("image_nx", 0), ("n_radial_bins", 0), ("radial_max", 0.0), ("image_x_max", -1.0)):
            p = params(rt, n, seed)
            setattr(p, field, value)
            refused(trace_rc(p, acc.data_ptr(), blk.data_ptr()))
        # a fraction within 2^-49 above 1 is accepted and stored as 1
        ok = good_rates.copy()
        ok[0, 3, 3] = 1.0 + 2.0 ** -50
        assert set_rc(ok, ones, 3, n_r, n_e) == 0
        assert rt.source_channels()[0, 3, 3] == 1.0
        # the channels go with the solar tables they belonged to
        L.check(lib.sart_set_solar_tables(h, L.as_dp(full.fluxRadiusCDF), L.as_dp(full.diffFluxCDFs), L.as_dp(full.energies), n_r, n_e))
        state.clear()
        refused(trace_rc(p_good, acc.data_ptr(), blk.data_ptr()), L.SART_ERR_NOT_READY)
        rt.synchronize()
        assert int(acc.abs().sum()) == 0 and int(blk.abs().sum()) == 0     # no refused launch wrote to the caller's buffers
    # the X-ray test source has no solar sampling
    with Tracer(make_setup("babyiaxo_xmm_xray")) as rt:
        lib, h = rt.lib, rt.handle
        rt.set_source_channels(good_rates, ones)
        f0 = rt.source_channels()
        s0 = L.Setup()
        L.check(lib.sart_get_setup(h, C.byref(s0)))
        _, sum0 = rt.trace_histogram(20_000, seed=seed)
        p = params(rt, 1000, seed)
        acc = zeros(torch, acc_len(rt, p), torch.float64)
        blk = zeros(torch, L.channel_block_len(3, n_e, True, 256, 256), torch.float64)
        with pytest.raises(L.SartError) as e:
            rt.trace_channels_device(p, acc.data_ptr(), blk.data_ptr())
        assert e.value.code == L.SART_ERR_INVALID_ARGUMENT and "test source" in str(e.value)
        s1 = L.Setup()
        L.check(lib.sart_get_setup(h, C.byref(s1)))
        assert bytes(s0) == bytes(s1)
        np.testing.assert_array_equal(rt.source_channels(), f0)
        sum1 = rt.trace_histogram(20_000, seed=seed)[1]
        assert {k: v for k, v in sum1.items() if k.startswith("N_")} == {k: v for k, v in sum0.items() if k.startswith("N_")}
        assert sum1["SUM_WEIGHTS"] == pytest.approx(sum0["SUM_WEIGHTS"], rel=1e-12)     # (f64 atomics: the order of the additions)
        assert float(acc.abs().sum()) == 0.0 and float(blk.abs().sum()) == 0.0


def test_cli_emission_channels_end_to_end(tmp_path):
    out = tmp_path / "a"
    r = subprocess.run([sys.executable, "-m", "solaraxionraytracing_amd", "--rays", "400000", "--outpath", str(out), "--emissionChannels",
                        "couplings"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "all-terms AGSS09 table made on the GPU" in r.stdout
    total = float([l for l in r.stdout.splitlines() if l.startswith("The total flux")][0].split()[-1])
    tab = R.read_flux_by_channel_csv(str(out / "flux_by_channel_IAXO.csv"))
    assert tab["name"] == list(R.COUPLINGS)
    assert tab["flux fraction"].sum() == pytest.approx(1.0, rel=1e-9)
    assert tab["flux"].sum() == pytest.approx(total, rel=1e-9)
    eb = np.loadtxt(out / "energies_by_channel_IAXO.csv", delimiter=",", skiprows=1, usecols=(0, 4), ndmin=2)
    for t, name in enumerate(R.COUPLINGS):
        z = np.loadtxt(out / ("axion_image_IAXO_%s.csv" % name), delimiter=",", skiprows=1, usecols=2)
        assert z.sum() == pytest.approx(tab["flux"][t], rel=1e-9), name
        assert eb[eb[:, 0] == t, 1].sum() == pytest.approx(tab["flux"][t], rel=1e-9), name
