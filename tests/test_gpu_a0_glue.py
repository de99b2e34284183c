"""Stage A0 and the loop glue of trace_histogram_kernel (csrc/sart_kernels.hip) against the same library with the stage switched
off (SART_NO_EARLY_REJECT: no stage A0, no ring 0, every pass goes straight to phase A), on the MI355X.

What the glue decides - which word of the shared stream belongs to which ray id, which chunks are cut by the launch's ends, which
dead rays count as having reached the telescope, where a survivor lands in ring 0, when the wave drains its rings and stops - shows in
the results only through WHICH rays are traced and counted.  In SART_ACCUM_FIXED64 every sum is an integer and does not depend on the
order of the additions, so image, scalars and spectra of the two forms are compared byte for byte: over launch sizes around the
wave, chunk and workgroup sizes, over offsets that cut the first and the last chunk, over split launches, setups and seeds."""
import os

import numpy as np
import pytest

import solaraxionraytracing_amd as sa
from solaraxionraytracing_amd import _lib as L
from tests.conftest import make_setup

pytestmark = pytest.mark.gpu

SETUPS = {
    "variant5": ("babyiaxo_xmm", {}),                               # constant path: stage A0 beside the LDS tile in ring 1's path column
    "carried_path": ("babyiaxo_xmm", {"SART_NO_PATH_CONST": "1"}),  # the form of a setup that fails path_is_constant: path in ring 1
    "gas": ("babyiaxo_xmm_gas", {}),
    "turned": ("babyiaxo_xmm_rot", {}),                             # turned telescope: zones with the tilt margin
    "cast_llnl_gold": ("cast_llnl_gold", {}),                       # telescope off the magnet axis: at most the zone of kind (a)
    "cast_abrixas": ("cast_abrixas", {}),
}
RAY_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1023, 4097, 100_003, 2_000_000)
OFFSETS = (0, 1, 3, 255, 257, 2**32 - 129)
SEEDS = (5, 2024)

_open = {}


def tracer(name, a0):
    """A context of setup `name` in FIXED64 mode, with stage A0 as the library builds it or switched off (the SART_* knobs are read
    when a context is created); kept open for the module."""
    key = (name, a0)
    if key not in _open:
        setup, env = SETUPS[name]
        env = dict(env)
        if not a0:
            env["SART_NO_EARLY_REJECT"] = "1"
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            rt = sa.RayTracer(make_setup(setup))
            rt.__enter__()
            rt.set_accumulation_mode("fixed64")
        finally:
            for k, v in old.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
        _open[key] = rt
    return _open[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for rt in _open.values():
        rt.__exit__(None, None, None)
    _open.clear()


def traced(rt, splits, seed, offset):
    """Image, scalars and spectra of the ray ids offset .. offset + sum(splits) as bytes, traced as accumulating launches."""
    off = offset
    for k, n in enumerate(splits):
        img, s, spec = rt.trace_spectra(n, seed=seed, ray_id_offset=off, accumulate=(k > 0), n_radial_bins=200, radial_max=10.0)
        off += n
    out = {"image": img.tobytes(), "scalars": np.array([s[k] for k in sorted(s)], dtype=np.float64).tobytes()}
    for k in sorted(spec):
        out["spectra/" + k] = np.ascontiguousarray(spec[k]).tobytes()
    return out, s


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], (what, k)


@pytest.mark.parametrize("name", list(SETUPS))
def test_every_launch_size_equals_stage_a0_off(name):
    on, off = tracer(name, True), tracer(name, False)
    for seed in SEEDS:
        for n in RAY_COUNTS:
            a, s = traced(on, (n,), seed, 0)
            b, _ = traced(off, (n,), seed, 0)
            assert s["N_RAYS"] == n
            assert_same(a, b, (name, seed, n))


@pytest.mark.parametrize("name", list(SETUPS))
def test_every_offset_equals_stage_a0_off(name):
    on, off = tracer(name, True), tracer(name, False)
    for ray_id_offset in OFFSETS:
        for n in (257, 4097):
            a, _ = traced(on, (n,), SEEDS[0], ray_id_offset)
            b, _ = traced(off, (n,), SEEDS[0], ray_id_offset)
            assert_same(a, b, (name, ray_id_offset, n))


@pytest.mark.parametrize("name", list(SETUPS))
def test_one_launch_equals_three_accumulating_launches(name):
    on, off = tracer(name, True), tracer(name, False)
    n = 100_003
    for ray_id_offset in (0, 255):
        one, s = traced(on, (n,), SEEDS[1], ray_id_offset)
        three, _ = traced(on, (1, n // 3 - 1, n - n // 3), SEEDS[1], ray_id_offset)   # cut at 1 and at N / 3
        assert s["N_PASSED"] > 0
        assert_same(one, three, (name, "split", ray_id_offset))
        assert_same(one, traced(off, (1, n // 3 - 1, n - n // 3), SEEDS[1], ray_id_offset)[0], (name, "split, stage A0 off", ray_id_offset))


def test_counters_equal_the_record_path():
    """The record kernel has no stage A0 and no rings: its per-ray flags, counted on the host."""
    rt = tracer("variant5", True)
    n = 200_000
    _, s = traced(rt, (n,), SEEDS[0], 0)
    rec = rt.traceAxionWrapper(n, seed=SEEDS[0])
    assert s["N_RAYS"] == n
    assert s["N_PASSED"] == int((rec["passed"] != 0).sum()) > 0.2 * n
    assert s["N_PASSED_TILL_WINDOW"] == int((rec["passedTillWindow"] != 0).sum())


def test_mass_scan_equals_stage_a0_off():
    """The fused 32-mass scan runs the same loop (constant-path instantiation with the scan accumulators in ring 1's path column)."""
    masses = np.linspace(0.0, 0.02, 32)
    res = []
    for a0 in (True, False):
        old = os.environ.get("SART_NO_EARLY_REJECT")
        if not a0:
            os.environ["SART_NO_EARLY_REJECT"] = "1"
        try:
            with sa.RayTracer(make_setup("babyiaxo_xmm_gas")) as rt:
                rt.set_accumulation_mode("fixed64")
                res.append([rt.trace_mass_scan(masses, n, seed=SEEDS[0]) for n in (65, 4097, 100_003)])
        finally:
            if not a0:
                if old is None:
                    del os.environ["SART_NO_EARLY_REJECT"]
                else:
                    os.environ["SART_NO_EARLY_REJECT"] = old
    for (pm_a, sh_a), (pm_b, sh_b) in zip(*res):
        for k in pm_a:
            assert np.asarray(pm_a[k]).tobytes() == np.asarray(pm_b[k]).tobytes(), k
        for k in sh_a:
            assert sh_a[k] == sh_b[k], k
