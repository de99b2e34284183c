"""The histogram kernel's 64 x 64 LDS image tile, its packed ring 1 and the phase-B gathers of the live lanes only (run on the
MI355X box).  All in SART_ACCUM_FIXED64 mode: integer accumulation does not depend on the order of the additions, so an image
that took the LDS tile must equal, bit for bit, the image of a context that accumulates with global atomics alone
(SART_NO_IMAGE_TILE=1), and every counter must equal what the records of the same rays give when counted on the host."""
import os

import numpy as np
import pytest

import solaraxionraytracing_amd as sa
from solaraxionraytracing_amd import _lib as L

pytestmark = pytest.mark.gpu

COUNTERS = ("N_RAYS", "N_PASSED", "N_PASSED_TILL_WINDOW", "N_HIT_NICKEL", "N_REACHED_TELESCOPE", "N_SHELL_SELECTED", "N_OUTSIDE_IMAGE")
SUMS = ("SUM_WEIGHTS", "SUM_X", "SUM_Y", "SUM_R", "SUM_WEIGHTS_SQ")
N = 20_000_000


def _with_env(env, fn):
    """fn() with the SART_* knobs of `env` set (they are read when a context is created)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _image(full, env, nx, ny, x_range, y_range):
    def go():
        with sa.RayTracer(full) as rt:
            rt.set_accumulation_mode("fixed64")
            return rt.trace_image(N, nx, ny, x_range=x_range, y_range=y_range, seed=5)
    return _with_env(env, go)


def _setup(name):
    if name == "babyiaxo_xmm":       # constant-path variant: tile = ring 1's path column + the cells behind the tables (64 x 64)
        return sa.initFullSetup()
    if name == "cast_llnl_gold":     # no stage A0: tile = ring 0 + the cells behind the tables (64 x 64)
        return sa.initFullSetup(L.ES_CAST, L.DK_INGRID2018, L.SK_VACUUM, L.TK_LLNL, reflectivity="gold")
    if name == "babyiaxo_xmm_gas":   # stage A0 on and the path carried: the cells behind the tables alone (45 x 45)
        return sa.initFullSetup(stage=L.SK_GAS)
    raise KeyError(name)


def _windows(full, cx, cy):
    """(name, nx, ny, x range, y range) around the spot's centroid (cx, cy): pixels of the default size (chip / 256) in every case."""
    s = full.setup
    px = s.chip_x_max / 256.0
    far_x = 0.0 if cx > 0.5 * s.chip_x_max else s.chip_x_max - 64 * px     # the corner of the chip away from the spot
    far_y = 0.0 if cy > 0.5 * s.chip_y_max else s.chip_y_max - 64 * px
    return [
        # the image begins in the middle of the focal spot: the tile is clamped to the image's corner, one half of the spot lies
        # outside the image and the other half runs across the tile's far edge
        ("straddling", 128, 128, (cx, cx + 128 * px), (cy - 10 * px, cy + 118 * px)),
        # the image is a corner of the chip away from the spot: the tile (clamped into the image) sees stray rays only
        ("outside", 64, 64, (far_x, far_x + 64 * px), (far_y, far_y + 64 * px)),
        # an image smaller than the tile: the tile is the whole image
        ("small", 40, 48, (cx - 20 * px, cx + 20 * px), (cy - 24 * px, cy + 24 * px)),
    ]


def _assert_same(a, b, what):
    (img_a, s_a), (img_b, s_b) = a, b
    assert np.array_equal(img_a.view(np.uint64), img_b.view(np.uint64)), (what, "image differs")
    for k in COUNTERS + SUMS:
        assert np.float64(s_a[k]).view(np.uint64) == np.float64(s_b[k]).view(np.uint64), (what, k, s_a[k], s_b[k])


@pytest.mark.parametrize("name", ["babyiaxo_xmm", "cast_llnl_gold", "babyiaxo_xmm_gas"])
def test_tile_image_equals_the_image_without_tile(name):
    full = _setup(name)
    s = full.setup
    default = (256, 256, (0.0, s.chip_x_max), (0.0, s.chip_y_max))
    img_t, s_t = _image(full, {}, *default)
    assert s_t["N_RAYS"] == N and s_t["N_PASSED"] > 1e5
    _assert_same((img_t, s_t), _image(full, {"SART_NO_IMAGE_TILE": "1"}, *default), (name, "default"))
    # the width knob (experiments: 56 = the tile before ring 1 was packed) changes nothing either
    _assert_same((img_t, s_t), _image(full, {"SART_IMAGE_TILE_MAX": "56"}, *default), (name, "56 wide"))
    # conservation: the image covers the chip, so it holds the weight of every passed ray
    assert s_t["N_OUTSIDE_IMAGE"] == 0 and img_t.sum() == pytest.approx(s_t["SUM_WEIGHTS"], rel=1e-12)
    cx, cy = s_t["SUM_X"] / s_t["N_PASSED"], s_t["SUM_Y"] / s_t["N_PASSED"]
    for what, nx, ny, xr, yr in _windows(full, cx, cy):
        a = _image(full, {}, nx, ny, xr, yr)
        _assert_same(a, _image(full, {"SART_NO_IMAGE_TILE": "1"}, nx, ny, xr, yr), (name, what))
        img, summ = a
        for k in COUNTERS[:6] + SUMS:        # the window changes the image and N_OUTSIDE_IMAGE only
            assert summ[k] == s_t[k], (name, what, k)
        assert summ["N_OUTSIDE_IMAGE"] > 0 and img.sum() < summ["SUM_WEIGHTS"], (name, what)
        if what == "straddling":
            assert img.sum() > 0.05 * summ["SUM_WEIGHTS"], (name, what)
        if what == "outside":
            assert img.sum() < 0.05 * summ["SUM_WEIGHTS"], (name, what)


def _counts_of_records(rec):
    return {"N_PASSED": int(rec["passed"].sum()), "N_PASSED_TILL_WINDOW": int(rec["passedTillWindow"].sum()),
            "N_HIT_NICKEL": int(rec["hitNickel"].sum())}


def _hist_vs_records(full, n, seed, offset=0):
    with sa.RayTracer(full) as rt:
        rec = rt.traceAxionWrapper(n, seed=seed, ray_id_offset=offset)
    with sa.RayTracer(full) as rt:
        rt.set_accumulation_mode("fixed64")
        img, summ = rt.trace_histogram(n, seed=seed, ray_id_offset=offset)
        quantum = rt.fixed_quanta()["weight"]
    want = _counts_of_records(rec)
    assert summ["N_RAYS"] == n
    for k, v in want.items():
        assert summ[k] == v, (k, summ[k], v)
    # every passed ray adds rint(weight / quantum): at most half a quantum of rounding per ray, beside the host's f64 sum of the
    # records (n additions of relative error 2^-53 each)
    w_rec = float(rec["weights"][rec["passed"] != 0].sum())
    assert abs(summ["SUM_WEIGHTS"] - w_rec) <= 0.5 * quantum * max(1, want["N_PASSED"]) + n * 2.0 ** -53 * abs(w_rec)
    assert img.sum() == pytest.approx(summ["SUM_WEIGHTS"], rel=1e-12) or summ["N_OUTSIDE_IMAGE"] > 0
    return summ, want


def test_counters_when_most_phase_b_rays_die():
    """Telescope tilted by 0.35 degrees: most rays that select a shell hit the nickel of the shell below or miss the second
    mirror, so most lanes of a phase-B pass are dead at the gathers."""
    full = sa.initFullSetup()
    full.setup.telescope_turned_y_deg = 0.35
    full.setup.chip_x_max = full.setup.chip_y_max = 100.0
    full.flags = L.CF_IGNORE_DET_WINDOW | L.CF_IGNORE_GAS_ABS | L.CF_IGNORE_CONV_PROB
    summ, want = _hist_vs_records(full, 400_000, seed=13)
    assert summ["N_SHELL_SELECTED"] > 50_000
    assert want["N_PASSED_TILL_WINDOW"] < 0.5 * summ["N_SHELL_SELECTED"]      # most phase-B rays die ...
    assert want["N_PASSED_TILL_WINDOW"] + want["N_HIT_NICKEL"] > 0            # ... but not all of them silently


@pytest.mark.parametrize("n,offset", [(1, 0), (37, 0), (63, 1000), (63, 255)])
def test_counters_of_a_launch_of_fewer_than_64_rays(n, offset):
    """One partial phase-B pass at most: the lanes beyond the valid rays run on the zeroed ring slots."""
    # the X-ray test source sends every ray through the bore, so even a handful of rays reaches phase B; the solar source as well
    for full in (sa.initFullSetup(), sa.initFullSetup(flags=L.CF_XRAY_TEST)):
        _hist_vs_records(full, n, seed=21, offset=offset)
