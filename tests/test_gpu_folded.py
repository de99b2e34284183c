"""The folded form of the constant-path histogram kernels (variants 7 / 8: folded_histogram_kernel, the wave-uniform switches of
variants 5 / 6 answered at compile time) against the run-time form of the same library (SART_NO_FOLDED=1).  The fold changes no
arithmetic and no lane assignment, so in SART_ACCUM_FIXED64 image and scalars are equal byte for byte, and in f64 mode the counters
and the five per-lane sums are equal to the last bit (the image's f64 atomics arrive in the order the hardware schedules the waves).
BabyIAXO / XMM in vacuum and with gas on the suite's small tables; launches of 1, 63, 64, 65, 257, 4097 and 200000 rays at three
ray_id_offsets; one launch against three accumulating launches cut at 1 and N / 3.  The query entry says which form a launch took:
folded for these, run-time for every launch one of whose answers is not the folded one - and those launches, too, give what their
SART_NO_FOLDED run gives."""
import ctypes as C
import os

import numpy as np
import pytest

import solaraxionraytracing_amd as sa
from solaraxionraytracing_amd import _lib as L
from tests.conftest import make_setup

pytestmark = pytest.mark.gpu

RAY_COUNTS = (1, 63, 64, 65, 257, 4097, 200_000)
OFFSETS = (0, 255, 2**32 - 129)
SEED = 5
FOLDED_SETUPS = ("babyiaxo_xmm", "babyiaxo_xmm_gas")

_open = {}


class _environment:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def tracer(name, no_folded, accumulation="fixed64", env=()):
    """A context of its own per setup, knob value, accumulation mode and further knobs (the SART_* knobs are read when a context is
    created); kept open for the module."""
    key = (name, no_folded, accumulation, tuple(env))
    if key not in _open:
        knobs = dict(env)
        if no_folded:
            knobs["SART_NO_FOLDED"] = "1"
        old = os.environ.pop("SART_NO_FOLDED", None)
        try:
            with _environment(knobs):
                rt = sa.RayTracer(make_setup(name))
                rt.__enter__()
                rt.set_accumulation_mode(accumulation)
        finally:
            if old is not None:
                os.environ["SART_NO_FOLDED"] = old
        _open[key] = rt
    return _open[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for rt in _open.values():
        rt.__exit__(None, None, None)
    _open.clear()


def form(rt):
    """1: the context's last histogram launch took the folded form, 0: the run-time form (internal query entry)."""
    fn = rt.lib.sart_internal_last_histogram_form
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p]
    return fn(rt.handle)


def packed(img, s):
    return {"image": img.tobytes(), "scalars": np.array([s[k] for k in sorted(s)], dtype=np.float64).tobytes()}


def same_bytes(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        assert got[k] == want[k], (what, k)


@pytest.mark.parametrize("name", FOLDED_SETUPS)
def test_fixed64_image_and_scalars_are_equal_byte_for_byte(name):
    folded, run_time = tracer(name, False), tracer(name, True)
    passed = 0
    for offset in OFFSETS:
        for n in RAY_COUNTS:
            img_f, s_f = folded.trace_histogram(n, seed=SEED, ray_id_offset=offset)
            img_r, s_r = run_time.trace_histogram(n, seed=SEED, ray_id_offset=offset)
            assert form(folded) == 1 and form(run_time) == 0, (name, offset, n)
            assert s_f["N_RAYS"] == n
            same_bytes(packed(img_f, s_f), packed(img_r, s_r), (name, offset, n))
            passed += s_f["N_PASSED"]
    assert passed > 0


@pytest.mark.parametrize("name", FOLDED_SETUPS)
def test_one_launch_equals_three_accumulating_launches(name):
    folded, run_time = tracer(name, False), tracer(name, True)
    for offset in OFFSETS:
        for n in (4097, 200_000):
            whole = packed(*folded.trace_histogram(n, seed=SEED, ray_id_offset=offset))
            cuts = (0, 1, n // 3, n)
            for rt, want_form in ((folded, 1), (run_time, 0)):
                for k in range(3):
                    img, s = rt.trace_histogram(cuts[k + 1] - cuts[k], seed=SEED, ray_id_offset=offset + cuts[k], accumulate=k > 0)
                    assert form(rt) == want_form
                assert s["N_RAYS"] == n and s["N_PASSED"] > 0
                same_bytes(packed(img, s), whole, (name, offset, n, want_form))


@pytest.mark.parametrize("name", FOLDED_SETUPS)
def test_f64_counters_and_sums_are_equal_to_the_last_bit(name):
    folded, run_time = tracer(name, False, "f64"), tracer(name, True, "f64")
    for offset in OFFSETS:
        for n in RAY_COUNTS:
            _, s_f = folded.trace_histogram(n, seed=SEED, ray_id_offset=offset)
            _, s_r = run_time.trace_histogram(n, seed=SEED, ray_id_offset=offset)
            assert form(folded) == 1 and form(run_time) == 0, (name, offset, n)
            assert s_f["N_RAYS"] == n
            for k in s_f:
                assert np.float64(s_f[k]).tobytes() == np.float64(s_r[k]).tobytes(), (name, offset, n, k, s_f[k], s_r[k])
    assert s_f["N_PASSED"] > 0 and s_f["SUM_WEIGHTS"] > 0.0


FOLDED_FLAGS = {"IGNORE_DET_WINDOW": L.CF_IGNORE_DET_WINDOW, "IGNORE_GAS_ABS": L.CF_IGNORE_GAS_ABS, "IGNORE_REFLECTION": L.CF_IGNORE_REFLECTION,
                "IGNORE_CONV_PROB": L.CF_IGNORE_CONV_PROB, "XRAY_TEST": L.CF_XRAY_TEST}


@pytest.mark.parametrize("name", FOLDED_SETUPS)
@pytest.mark.parametrize("flag", list(FOLDED_FLAGS))
def test_a_folded_flag_set_alone_takes_the_run_time_form(name, flag):
    folded, run_time = tracer(name, False), tracer(name, True)
    img_f, s_f = folded.trace_histogram(20_000, seed=SEED, flags=FOLDED_FLAGS[flag])
    assert form(folded) == 0
    img_r, s_r = run_time.trace_histogram(20_000, seed=SEED, flags=FOLDED_FLAGS[flag])
    assert form(run_time) == 0 and s_f["N_PASSED"] > 0
    same_bytes(packed(img_f, s_f), packed(img_r, s_r), (name, flag))
    # ... and the launch behind it, without the flag, is folded again
    folded.trace_histogram(4097, seed=SEED)
    assert form(folded) == 1


@pytest.mark.parametrize("name", FOLDED_SETUPS)
def test_spectra_take_the_run_time_form(name):
    folded, run_time = tracer(name, False), tracer(name, True)
    got = folded.trace_spectra(20_000, seed=SEED, n_radial_bins=200, radial_max=10.0)
    assert form(folded) == 0
    want = run_time.trace_spectra(20_000, seed=SEED, n_radial_bins=200, radial_max=10.0)
    assert form(run_time) == 0 and got[1]["N_PASSED"] > 0
    same_bytes(packed(got[0], got[1]), packed(want[0], want[1]), name)
    for k in want[2]:
        assert np.ascontiguousarray(got[2][k]).tobytes() == np.ascontiguousarray(want[2][k]).tobytes(), (name, k)


# context, setup of the suite, knobs: every one has an answer that is not the folded one
RUN_TIME_CONTEXTS = {
    "SART_ENERGY_RECORDS=0": ("babyiaxo_xmm", {"SART_ENERGY_RECORDS": "0"}),
    "SART_NO_RADIAL_TABLE=1": ("babyiaxo_xmm", {"SART_NO_RADIAL_TABLE": "1"}),
    "SART_NO_EARLY_REJECT=1": ("babyiaxo_xmm", {"SART_NO_EARLY_REJECT": "1"}),
    "cast_llnl": ("cast_llnl_gold", {}),
    "cast_abrixas": ("cast_abrixas", {}),
    "xray_source": ("babyiaxo_xmm_xray", {}),
    "turned_telescope": ("babyiaxo_xmm_rot", {}),
}


@pytest.mark.parametrize("case", list(RUN_TIME_CONTEXTS))
def test_other_contexts_take_the_run_time_form(case):
    name, env = RUN_TIME_CONTEXTS[case]
    a, b = tracer(name, False, env=tuple(sorted(env.items()))), tracer(name, True, env=tuple(sorted(env.items())))
    img_a, s_a = a.trace_histogram(20_000, seed=SEED)
    img_b, s_b = b.trace_histogram(20_000, seed=SEED)
    assert form(a) == 0 and form(b) == 0, case
    assert s_a["N_RAYS"] == 20_000 and s_a["N_REACHED_TELESCOPE"] > 0
    same_bytes(packed(img_a, s_a), packed(img_b, s_b), case)


def test_no_launch_yet_and_the_default_is_folded():
    old = os.environ.pop("SART_NO_FOLDED", None)
    try:
        with sa.RayTracer(make_setup("babyiaxo_xmm")) as rt:
            assert form(rt) == -1
            rt.trace_histogram(4097, seed=SEED)
            assert form(rt) == 1
    finally:
        if old is not None:
            os.environ["SART_NO_FOLDED"] = old
