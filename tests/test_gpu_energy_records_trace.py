"""The energy draw through the bucket records (SART_ENERGY_RECORDS=1) against the two-level draw (SART_ENERGY_RECORDS=0) in the
accumulating kernels: the draw gives the same index for every ray, so in SART_ACCUM_FIXED64 image, scalars and spectra are equal byte
for byte, and in f64 mode the counters and the five per-lane sums are equal to the last bit (the image's f64 atomics arrive in the
order the hardware schedules the waves, which no draw fixes; the scans' f64 sums: see _same).  Launches of 1, 63, 64, 65, 4097 and 200000 rays, two ray_id_offsets;
the headline kernel (variant 5), its carried-path form, gas, the telescope turned by 0.1 degrees, CAST / LLNL with gold and with its
four coatings, the 32-mass scan and its banded form, the 16-angle scan."""
import ctypes as C
import os

import numpy as np
import pytest

import solaraxionraytracing_amd as sa
from tests.conftest import make_setup

pytestmark = pytest.mark.gpu

SETUPS = {
    "variant5": ("babyiaxo_xmm", {}),
    "carried_path": ("babyiaxo_xmm", {"SART_NO_PATH_CONST": "1"}),
    "gas": ("babyiaxo_xmm_gas", {}),
    "turned_0.1deg": ("babyiaxo_xmm_rot", {}),
    "cast_llnl_gold": ("cast_llnl_gold", {}),
    "cast_llnl_four_coatings": ("cast_llnl", {}),
}
RAY_COUNTS = (1, 63, 64, 65, 4097, 200_000)
OFFSETS = (0, 2**32 - 129)
SEED = 5

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


def _full(name):
    full = make_setup(SETUPS[name][0])
    if name == "turned_0.1deg":
        full.setup.telescope_turned_x_deg, full.setup.telescope_turned_y_deg = 0.0, 0.1
    return full


def tracer(name, records, accumulation="fixed64"):
    """A context of its own per setup, knob value and accumulation mode (the SART_* knobs are read when a context is created and
    when it receives its tables); kept open for the module."""
    key = (name, records, accumulation)
    if key not in _open:
        with _environment({**SETUPS[name][1], "SART_ENERGY_RECORDS": str(records)}):
            rt = sa.RayTracer(_full(name))
            rt.__enter__()
            rt.set_accumulation_mode(accumulation)
        _open[key] = rt
    return _open[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for rt in _open.values():
        rt.__exit__(None, None, None)
    _open.clear()


def traced(rt, n, offset):
    img, s, spec = rt.trace_spectra(n, seed=SEED, ray_id_offset=offset, n_radial_bins=200, radial_max=10.0)
    out = {"image": img.tobytes(), "scalars": np.array([s[k] for k in sorted(s)], dtype=np.float64).tobytes()}
    for k in sorted(spec):
        out["spectra/" + k] = np.ascontiguousarray(spec[k]).tobytes()
    return out, s


@pytest.mark.parametrize("name", list(SETUPS))
def test_fixed64_image_scalars_and_spectra_are_equal_byte_for_byte(name):
    passed = 0
    for offset in OFFSETS:
        for n in RAY_COUNTS:
            off, s = traced(tracer(name, 0), n, offset)
            on, _ = traced(tracer(name, 1), n, offset)
            assert s["N_RAYS"] == n and off.keys() == on.keys()
            for k in off:
                assert off[k] == on[k], (name, offset, n, k)
            passed += s["N_PASSED"]
    assert passed > 0


@pytest.mark.parametrize("name", list(SETUPS))
def test_f64_counters_and_sums_are_equal_to_the_last_bit(name):
    a, b = tracer(name, 0, "f64"), tracer(name, 1, "f64")
    for offset in OFFSETS:
        for n in RAY_COUNTS:
            _, s0 = a.trace_histogram(n, seed=SEED, ray_id_offset=offset)
            _, s1 = b.trace_histogram(n, seed=SEED, ray_id_offset=offset)
            assert s0["N_RAYS"] == n
            for k in s0:
                assert np.float64(s0[k]).tobytes() == np.float64(s1[k]).tobytes(), (name, offset, n, k, s0[k], s1[k])
    assert s0["N_PASSED"] > 0 and s0["SUM_WEIGHTS"] > 0.0


def records_on(rt):
    """HotB::records_on as the context's next launch carries it (internal query entry)."""
    fn = rt.lib.sart_internal_energy_records
    fn.restype = C.c_int
    on = fn(rt.handle)
    assert on in (0, 1)
    return on


def test_the_knob_sets_the_switch():
    """Without this every comparison below could pass with both contexts on one path: SART_ENERGY_RECORDS=1 runs with records, =0
    without, the default is the documented one (on), and a table of more than 2047 energies runs without whatever the knob says."""
    for name in SETUPS:
        for accumulation in ("fixed64", "f64"):
            assert records_on(tracer(name, 1, accumulation)) == 1 and records_on(tracer(name, 0, accumulation)) == 0, (name, accumulation)
    old = os.environ.pop("SART_ENERGY_RECORDS", None)
    try:
        with sa.RayTracer(make_setup("babyiaxo_xmm")) as rt:
            assert records_on(rt) == 1
    finally:
        if old is not None:
            os.environ["SART_ENERGY_RECORDS"] = old
    with _environment({"SART_ENERGY_RECORDS": "1"}):
        with sa.RayTracer(make_setup("babyiaxo_xmm", n_energies=2048)) as rt:       # one energy more than a record's lo can index
            assert records_on(rt) == 0
            _, s = rt.trace_histogram(4097, seed=SEED)
            assert s["N_RAYS"] == 4097
        with sa.RayTracer(make_setup("babyiaxo_xmm", n_energies=2047)) as rt:       # the largest table a record's lo can index
            assert records_on(rt) == 1


def _same(got, want, what, exact):
    """exact: byte for byte (FIXED64).  The issue asks for the f64 sums bit for bit; the histogram launches above meet that, the
    scans cannot: they add a workgroup's rays into LDS cells shared by its 16 waves with f64 atomics, in the order the waves arrive,
    so two runs of ONE library differ in the last bits already (tests/test_gpu_mass_scan.py, tests/test_gpu_angular_scan.py).  Their
    f64 sums are held to what those suites hold the same quantities to, 1e-12 on the sums of the weights and 1e-11 on the sums of
    their squares, and every counter (integers) exactly."""
    for d_got, d_want in zip(got, want):
        assert d_got.keys() == d_want.keys()
        for k in d_want:
            a, b = np.asarray(d_got[k]), np.asarray(d_want[k])
            if exact or not k.startswith("SUM_"):
                assert a.tobytes() == b.tobytes(), (what, k)
            else:
                assert np.all(np.abs(a - b) <= (1e-11 if k.startswith("SUM_WEIGHTS_SQ") else 1e-12) * np.abs(b)), (what, k)


@pytest.mark.parametrize("accumulation", ["fixed64", "f64"])
def test_mass_scan_and_its_banded_form(accumulation):
    masses = np.linspace(0.0, 0.02, 32)
    res = {}
    for records in (0, 1):
        with _environment({"SART_ENERGY_RECORDS": str(records)}):
            with sa.RayTracer(make_setup("babyiaxo_xmm_gas")) as rt:
                rt.set_accumulation_mode(accumulation)
                res[records] = [rt.trace_mass_scan(masses, n, seed=SEED, ray_id_offset=offset) for offset in OFFSETS for n in RAY_COUNTS]
                assert records_on(rt) == records
                res[records] += [rt.trace_mass_scan_spectra(masses, (0, 10, 8), n, seed=SEED, ray_id_offset=offset)
                                 for offset in OFFSETS for n in RAY_COUNTS]
    assert res[0][5][0]["SUM_WEIGHTS"].max() > 0.0
    for k, (got, want) in enumerate(zip(res[1], res[0])):
        _same(got, want, ("mass scan", accumulation, k), accumulation == "fixed64")


@pytest.mark.parametrize("accumulation", ["fixed64", "f64"])
def test_angular_scan_of_16_angles(accumulation):
    angles = np.linspace(0.0, 0.15, 16)
    res = {}
    for records in (0, 1):
        with _environment({"SART_ENERGY_RECORDS": str(records)}):
            with sa.RayTracer(make_setup("babyiaxo_xmm")) as rt:
                rt.set_accumulation_mode(accumulation)
                assert records_on(rt) == records
                res[records] = [rt.trace_angular_scan(angles, n, seed=SEED, ray_id_offset=offset) for offset in OFFSETS for n in RAY_COUNTS]
    assert res[0][5][0]["SUM_WEIGHTS"].max() > 0.0
    for k, (got, want) in enumerate(zip(res[1], res[0])):
        _same(got, want, ("angular scan", accumulation, k), accumulation == "fixed64")
