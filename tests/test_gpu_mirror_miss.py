"""The mirror-miss shortcut of trace_histogram_kernel (DevParams::mirror_miss_radius; run on the MI355X box).

Phase A ends a ray that provably misses the first mirror of a shell above the innermost one and provably hits the nickel of the
shell below: +1 in N_HIT_NICKEL is all phase B would have made of it.  Exactness is tested three ways: bitwise against the
launch with the shortcut switched off (SART_NO_SURE_MISS), counter for counter against the record path (which runs the whole
of phase B for every ray), and through the diagnostic kernel behind sart_internal_mirror_miss, which evaluates the shortcut's
predicate beside phase B's own first-mirror arithmetic and counts contradictions."""
import ctypes as C
import os

import numpy as np
import pytest

import solaraxionraytracing_amd as sa
from solaraxionraytracing_amd import _lib as L

pytestmark = pytest.mark.gpu

SMALL = dict(n_radii=400, n_energies=300, refl_n_angles=200, refl_n_energies=200)
COUNTERS = ("N_RAYS", "N_PASSED", "N_PASSED_TILL_WINDOW", "N_HIT_NICKEL", "N_REACHED_TELESCOPE", "N_SHELL_SELECTED", "N_OUTSIDE_IMAGE")
SUMS = ("SUM_WEIGHTS", "SUM_X", "SUM_Y", "SUM_R", "SUM_WEIGHTS_SQ")

_cache = {}


def full_setup(name):
    if name not in _cache:
        if name == "babyiaxo_xmm":
            full = sa.initFullSetup(**SMALL)
        elif name == "babyiaxo_xmm_gas":
            full = sa.initFullSetup(stage=L.SK_GAS, **SMALL)
        elif name == "cast_abrixas_gas":
            full = sa.initFullSetup(L.ES_CAST, L.DK_INGRID2017, L.SK_GAS, L.TK_ABRIXAS, **SMALL)
        elif name == "cast_llnl_gold":
            full = sa.initFullSetup(L.ES_CAST, L.DK_INGRID2018, L.SK_VACUUM, L.TK_LLNL, reflectivity="gold", **SMALL)
        elif name == "babyiaxo_xmm_xray":
            full = sa.initFullSetup(flags=L.CF_XRAY_TEST, **SMALL)
        elif name == "babyiaxo_xmm_rot":
            full = sa.initFullSetup(**SMALL)
            full.setup.telescope_turned_y_deg = 0.1
            full.setup.chip_x_max = full.setup.chip_y_max = 100.0
            full.flags = L.CF_IGNORE_DET_WINDOW | L.CF_IGNORE_GAS_ABS | L.CF_IGNORE_CONV_PROB
        else:
            raise KeyError(name)
        _cache[name] = full
    return _cache[name]


class _env:
    def __init__(self, env):
        self.env = env or {}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def mirror_miss(full, env=None, n_rays=0, seed=5):
    """(radius, slope_sq, thresholds[n_shells], counts[5] or None) of sart_internal_mirror_miss in a fresh context."""
    with _env(env), sa.RayTracer(full) as rt:
        fn = rt.lib.sart_internal_mirror_miss
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(L.TraceParams), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        radius, slope_sq = C.c_double(), C.c_double()
        thr = (C.c_double * int(full.setup.n_shells))()
        counts = (C.c_uint64 * 5)()
        p = rt.trace_params(n_rays, seed=seed) if n_rays else None
        L.check(fn(rt.handle, C.byref(p) if p is not None else None, C.byref(radius), C.byref(slope_sq), thr, counts if n_rays else None))
        return radius.value, slope_sq.value, np.array(thr[:]), (np.array(counts[:], dtype=np.int64) if n_rays else None)


def histogram(name, seed, env=None, n=2_000_000):
    with _env(env), sa.RayTracer(full_setup(name)) as rt:
        rt.set_accumulation_mode("fixed64")
        return rt.trace_histogram(n, seed=seed)


@pytest.mark.parametrize("seed", [5, 6])
@pytest.mark.parametrize("name,env", [("babyiaxo_xmm", {}), ("babyiaxo_xmm", {"SART_NO_PATH_CONST": "1"}), ("babyiaxo_xmm_gas", {}),
                                      ("cast_abrixas_gas", {}), ("babyiaxo_xmm_rot", {})])
def test_bitwise_equal_with_and_without_the_shortcut(name, env, seed):
    """A ray wrongly ended moves N_PASSED or a pixel, a wrong verdict moves N_HIT_NICKEL: the whole FIXED64 accumulator is compared
    byte for byte (variant 5, variant 0 through SART_NO_PATH_CONST, gas, the other Wolter telescope, the turned telescope)."""
    on = histogram(name, seed, env)
    off = histogram(name, seed, dict(env, SART_NO_SURE_MISS="1"))
    assert on[1]["N_HIT_NICKEL"] > 0 and on[1]["N_PASSED"] > 1000
    assert on[0].tobytes() == off[0].tobytes()
    for k in COUNTERS + SUMS:
        assert np.float64(on[1][k]).tobytes() == np.float64(off[1][k]).tobytes(), (k, on[1][k], off[1][k])


@pytest.mark.parametrize("name", ["babyiaxo_xmm", "cast_abrixas_gas"])
def test_counters_equal_those_of_the_record_path(name):
    n = 200_000
    with sa.RayTracer(full_setup(name)) as rt:
        rec = rt.traceAxionWrapper(n, seed=11)
        _, summ = rt.trace_histogram(n, seed=11)
    assert summ["N_HIT_NICKEL"] == int(rec["hitNickel"].sum()) > 0
    assert summ["N_PASSED"] == int(rec["passed"].sum())
    assert summ["N_PASSED_TILL_WINDOW"] == int(rec["passedTillWindow"].sum())


def test_thresholds_where_they_are_proved_and_only_there():
    full = full_setup("babyiaxo_xmm")
    r1 = np.array(full.setup.all_r1[:full.setup.n_shells])
    radius, slope_sq, thr, _ = mirror_miss(full)
    print("mirror_miss_radius", radius, "slope bound", np.sqrt(slope_sq), "shells with a threshold", int(np.isfinite(thr).sum()), "of", len(thr))
    assert np.isfinite(radius) and np.any(np.abs(radius - r1[:-1]) < 1e-4)   # R1 of a shell, rounded up to a float
    # the slope bound: at most the largest slope of a ray from the Sun (9.3e-4 with these tables' 400 radii, 4.6e-3 with the full
    # table), at least 0.4 of it (below that the host drops the shell)
    assert 3.7e-4 < np.sqrt(slope_sq) < 9.3e-4
    assert thr[0] == -np.inf                                   # the innermost shell has its own shortcut
    on = np.isfinite(thr)
    assert on[-1] and on.sum() >= len(thr) // 2                # the outer shells
    assert np.array_equal(on[1:], r1[1:] > radius)             # exactly the shells above the radius
    assert np.all(thr[on] < r1[on] ** 2) and np.all(thr[on] > 0.0)
    g_radius, g_slope_sq, g_thr, _ = mirror_miss(full_setup("babyiaxo_xmm_gas"))
    assert g_radius == radius and g_slope_sq == slope_sq and np.array_equal(g_thr, thr)   # the stage does not enter
    for name, env in (("cast_llnl_gold", None), ("babyiaxo_xmm_xray", None), ("babyiaxo_xmm_rot", None),
                      ("babyiaxo_xmm", {"SART_NO_SURE_MISS": "1"}), ("babyiaxo_xmm", {"SART_NO_EARLY_REJECT": "1"})):
        radius_n, _, thr_n, _ = mirror_miss(full_setup(name), env)
        assert radius_n == np.inf and np.all(thr_n == -np.inf), (name, env)


def test_share_of_the_missed_rays_the_shortcut_ends():
    """Measured on the MI355X with these tables, 2e6 rays, seed 5: 74392 of the 74409 rays that miss the first mirror of a shell above
    the innermost (167224 with the innermost shell's) - SHARE_MEASURED, the run that wrote it down; the floor is that figure minus
    five standard deviations of a binomial sample of the missed rays.  With the full solar table (1968 radii, 2e7 rays): 743075 of
    743862, 0.9989, the slope bound 2.65e-3 of 4.55e-3; cast_abrixas_gas 901655 of 902449."""
    n = 2_000_000
    _, _, _, counts = mirror_miss(full_setup("babyiaxo_xmm"), n_rays=n, seed=5)
    missed, missed_upper, sure, sure_hit, sure_no_nickel = (int(x) for x in counts)
    share = sure / max(missed_upper, 1)
    print("missed mirror 1: %d (above the innermost shell %d), ended by the shortcut %d, share %.4f" % (missed, missed_upper, sure, share))
    assert sure_hit == 0 and sure_no_nickel == 0               # what the host's two proofs exclude
    assert sure <= missed_upper <= missed
    with sa.RayTracer(full_setup("babyiaxo_xmm")) as rt:       # the histogram's nickel counter holds them all
        assert rt.trace_histogram(n, seed=5)[1]["N_HIT_NICKEL"] >= sure
    floor = SHARE_MEASURED - 5.0 * np.sqrt(SHARE_MEASURED * (1.0 - SHARE_MEASURED) / missed_upper)
    assert share >= floor, (share, floor)


SHARE_MEASURED = 74392 / 74409
