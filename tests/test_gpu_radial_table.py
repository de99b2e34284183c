"""The radial verdict table of the solar-source histogram kernels on the GPU (run on the MI355X box).

Stage A1 takes everything the radial distance at the entrance plane decides - inner disc, XMM ring, last shell, shell selection,
glass front, the two sure-miss radii - from one table lookup (csrc/sart_device.h: RadialLds).  Exactness is tested four ways: the
library's table against the numpy model, and both device forms of the verdict on crafted radii (sart_internal_radial_verdicts);
whole FIXED64 accumulators with spectra byte for byte against the launch that runs the compares (SART_NO_RADIAL_TABLE); counters
against the record path; a setup whose cells are marked."""
import ctypes as C
import os

import numpy as np
import pytest

import solaraxionraytracing_amd as sa
from solaraxionraytracing_amd import _lib as L
from tests.radial_table_model import Geo, MARKED, crafted_radii

pytestmark = pytest.mark.gpu

SMALL = dict(n_radii=400, n_energies=300, refl_n_angles=200, refl_n_energies=200)
COUNTERS = ("N_RAYS", "N_PASSED", "N_PASSED_TILL_WINDOW", "N_HIT_NICKEL", "N_REACHED_TELESCOPE", "N_SHELL_SELECTED", "N_OUTSIDE_IMAGE")
SUMS = ("SUM_WEIGHTS", "SUM_X", "SUM_Y", "SUM_R", "SUM_WEIGHTS_SQ")
OFF = {"SART_NO_RADIAL_TABLE": "1"}

_cache = {}


def full_setup(name):
    if name not in _cache:
        if name == "babyiaxo_xmm":
            full = sa.initFullSetup(**SMALL)
        elif name == "babyiaxo_xmm_gas":
            full = sa.initFullSetup(stage=L.SK_GAS, **SMALL)
        elif name == "cast_abrixas":
            full = sa.initFullSetup(L.ES_CAST, L.DK_INGRID2017, L.SK_VACUUM, L.TK_ABRIXAS, **SMALL)
        elif name == "cast_llnl_gold":
            full = sa.initFullSetup(L.ES_CAST, L.DK_INGRID2018, L.SK_VACUUM, L.TK_LLNL, reflectivity="gold", **SMALL)
        elif name == "babyiaxo_xmm_rot":
            full = sa.initFullSetup(**SMALL)
            full.setup.telescope_turned_y_deg = 0.1
            full.setup.chip_x_max = full.setup.chip_y_max = 100.0
            full.flags = L.CF_IGNORE_DET_WINDOW | L.CF_IGNORE_GAS_ABS | L.CF_IGNORE_CONV_PROB
        elif name == "babyiaxo_xmm_thick":
            # the glass of two shells thickened to within 2e-4 mm of the next shell: two breakpoints that the look-up table's step
            # (bounded below by r_last / 1022) cannot separate - their cells are marked and their lanes evaluate the compares
            full = sa.initFullSetup(**SMALL)
            s = full.setup
            for j in (20, 40):
                s.all_thickness[j] = s.all_r1[j + 1] - s.all_r1[j] - 2e-4
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


def sure_miss_radii(rt):
    """(shell0_miss_radius, mirror_miss_radius) of the context's next launch."""
    f0 = rt.lib.sart_internal_shell0_miss_radius
    f0.restype, f0.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_double)]
    shell0 = C.c_double()
    L.check(f0(rt.handle, C.byref(shell0)))
    f1 = rt.lib.sart_internal_mirror_miss
    f1.restype = C.c_int
    f1.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p, C.c_void_p]
    radius, slope_sq = C.c_double(), C.c_double()
    L.check(f1(rt.handle, None, C.byref(radius), C.byref(slope_sq), None, None))
    return shell0.value, radius.value


def device_verdicts(rt, radii):
    fn = rt.lib.sart_internal_radial_verdicts
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    radii = np.ascontiguousarray(radii, dtype=np.float64)
    a, b = np.empty(radii.size, dtype=np.uint32), np.empty(radii.size, dtype=np.uint32)
    L.check(fn(rt.handle, radii.ctypes.data_as(C.c_void_p), radii.size, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)))
    return a, b


@pytest.mark.parametrize("name", ["babyiaxo_xmm", "cast_llnl_gold", "cast_abrixas", "babyiaxo_xmm_rot", "babyiaxo_xmm_thick"])
def test_table_equals_the_model_and_both_device_forms_agree(name):
    full = full_setup(name)
    with sa.RayTracer(full) as rt:
        shell0, mirror = sure_miss_radii(rt)
        lib_table = rt.radial_table()
        assert lib_table is not None, "the shipped telescopes get a table"
        g = Geo(full.setup, shell0, mirror, rotated=name.endswith("_rot"))
        table = g.build()
        assert table is not None
        for got, want, what in zip(lib_table, table, ("breakpoints", "verdict words", "cells")):
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), what
        n_marked = int((table[2] == MARKED).sum())
        print(name, "entries", len(table[0]), "cells", len(table[2]), "marked", n_marked, "shell0_miss", shell0, "mirror_miss", mirror)
        assert (n_marked > 1) == (name == "babyiaxo_xmm_thick")   # one breakpoint per cell for the shipped telescopes (cell 0 apart)
        # 4096 crafted radii: every breakpoint and its neighbours, the edges of the cells around them, the special values, uniform ones
        r = crafted_radii(g, table, 0)
        assert r.size <= 4096
        r = np.concatenate([r, np.random.default_rng(3).uniform(0.0, 1.05 * g.r_last, 4096 - r.size)])
        by_table, by_compares = device_verdicts(rt, r)
    want = g.by_compares(r)
    assert np.array_equal(by_compares, want), "the device's compares against the model's"
    bad = np.nonzero(by_table != by_compares)[0]
    assert bad.size == 0, (r[bad[:5]], by_table[bad[:5]], by_compares[bad[:5]])
    assert len(np.unique(want >> 6)) >= 2 and len(np.unique(want & 63)) == full.setup.n_shells


def histogram(name, seed, env=None, n=2_000_000):
    with _env(env), sa.RayTracer(full_setup(name)) as rt:
        rt.set_accumulation_mode("fixed64")
        table = rt.radial_table() is not None
        return rt.trace_spectra(n, seed=seed, n_radial_bins=1000) + (table,)


def same_bytes(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(same_bytes(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same_bytes(x, y) for x, y in zip(a, b))
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.mark.parametrize("seed", [5, 6])
@pytest.mark.parametrize("name,env", [("babyiaxo_xmm", {}), ("babyiaxo_xmm", {"SART_NO_PATH_CONST": "1"}), ("babyiaxo_xmm_gas", {}),
                                      ("babyiaxo_xmm_rot", {}), ("cast_llnl_gold", {}), ("cast_abrixas", {}), ("babyiaxo_xmm_thick", {})])
def test_bitwise_equal_with_and_without_the_table(name, env, seed):
    """The whole FIXED64 accumulator with spectra, byte for byte (variant 5, variant 0 through SART_NO_PATH_CONST, gas, the turned
    telescope, the cone telescope, the off-axis Wolter one, and the setup with marked cells)."""
    on = histogram(name, seed, env)
    off = histogram(name, seed, dict(env, **OFF))
    assert on[-1] and not off[-1]
    assert on[1]["N_PASSED"] > 1000 and on[1]["N_SHELL_SELECTED"] > on[1]["N_PASSED"]
    assert same_bytes(on[:-1], off[:-1])
    for k in COUNTERS + SUMS:
        assert np.float64(on[1][k]).tobytes() == np.float64(off[1][k]).tobytes(), (k, on[1][k], off[1][k])


@pytest.mark.parametrize("name", ["babyiaxo_xmm", "cast_abrixas", "cast_llnl_gold"])
def test_counters_equal_those_of_the_record_path(name):
    n = 200_000
    with sa.RayTracer(full_setup(name)) as rt:
        assert rt.radial_table() is not None
        rec = rt.traceAxionWrapper(n, seed=11)
        _, summ = rt.trace_histogram(n, seed=11)
    assert summ["N_HIT_NICKEL"] == int(rec["hitNickel"].sum())
    assert summ["N_PASSED"] == int(rec["passed"].sum()) > 0
    assert summ["N_PASSED_TILL_WINDOW"] == int(rec["passedTillWindow"].sum())
