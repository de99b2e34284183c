"""The wide pass of stage A0 (csrc/sart_trace_histogram.inc: two words of a lane's stream block per loop iteration where ring 0 has
room) on the MI355X: the same library with SART_A0_WIDE = 0 (the one-word loop), 1 (the host's rule, sart_api.hip: a0_wide_rule), 2
(wide wherever zones exist) and with stage A0 switched off altogether (SART_NO_EARLY_REJECT).

The wide pass only changes HOW OFTEN the loop's glue runs: every ray still enters ring 0 once, in the order of the one-word loop, so
it reaches the same lane of the same phase-A and phase-B pass.  In SART_ACCUM_FIXED64 every sum is an integer, and image, scalars
and spectra are compared byte for byte; in f64 mode the counters and the five per-lane sums must be equal to the last bit between
SART_A0_WIDE = 0 and 2 (the image's f64 atomics arrive in the order the hardware schedules the waves, which no loop fixes).

The fall-back (a second word whose survivors do not fit ring 0, taken again by the next pass) is rare where the rule switches the
wide pass on: 0.6 % of the even passes on BabyIAXO / XMM at the tests' table sizes (the zones cover 0.543 of the words).
SART_A0_WIDE=2 switches the wide pass on wherever zones exist.  Of the setups the suite traces, the one with zones that cover least
is BabyIAXO / XMM turned by 40 degrees (tests/test_gpu_parity.py: no zone of the entrance plane survives that tilt, the pipes' zone
alone is left): it covers 0.451 of the words, stage A0 hands on FORCED_SURVIVAL = 0.549 of the rays, and the model
(a0_wide_fallback_share) has FORCED_SHARE = 0.102 of the even passes fall back - every tenth one, some 1600 fall-backs in a launch of
2e6 rays, 0 to 2 per wave in the small launches.  (That is still below the 1/8 at which the rule switches the wide pass off: no
setup with zones lies above it, the CPU model covers those survival rates.)"""
import ctypes as C
import os

import numpy as np
import pytest

import solaraxionraytracing_amd as sa
from tests.conftest import make_setup

pytestmark = pytest.mark.gpu

SETUPS = {
    "variant5": ("babyiaxo_xmm", {}),                               # constant path: the headline kernel
    "carried_path": ("babyiaxo_xmm", {"SART_NO_PATH_CONST": "1"}),  # the form of a setup that fails path_is_constant
    "gas": ("babyiaxo_xmm_gas", {}),
    "turned": ("babyiaxo_xmm_rot", {}),                             # turned telescope: zones with the tilt margin
    "cast_llnl_gold": ("cast_llnl_gold", {}),                       # telescope off the magnet axis: no zones, no wide pass
    "turned_40deg": ("babyiaxo_xmm_rot", {}),                       # the forced fall-backs: the pipes' zone alone
}
FORCED = "turned_40deg"
FORCED_SURVIVAL = 0.5490   # the share of the words its one zone leaves
FORCED_SHARE = 0.1024      # a0_wide_fallback_share(FORCED_SURVIVAL)
MODES = ("wide0", "wide1", "wide2", "a0_off")
RAY_COUNTS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 1023, 1025, 2_000_000)
OFFSETS = (0, 1, 2, 3, 127, 129, 255, 257, 2**32 - 129)
SEEDS = (5, 2024)

_open = {}


def _env_of(mode):
    return {"SART_NO_EARLY_REJECT": "1"} if mode == "a0_off" else {"SART_A0_WIDE": mode[-1]}


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


def tracer(name, mode, accumulation="fixed64"):
    """A context of its own per setup, knob value and accumulation mode (the SART_* knobs are read when a context is created); kept
    open for the module."""
    key = (name, mode, accumulation)
    if key not in _open:
        setup, env = SETUPS[name]
        full = make_setup(setup)
        if name == FORCED:
            full.setup.telescope_turned_y_deg = 40.0
        with _environment({**env, **_env_of(mode)}):
            rt = sa.RayTracer(full)
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


def wide_switch(rt):
    """(the switch a launch of this context carries, the survival rate of stage A0 its zones leave)"""
    fn = rt.lib.sart_internal_a0_wide
    fn.restype = C.c_int
    s = C.c_double()
    on = fn(rt.handle, C.byref(s))
    assert on >= 0
    return on, s.value


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


def test_the_knob_sets_the_switch_and_the_rule_follows_the_zones():
    share = sa._lib.load_sart().sart_internal_a0_wide_share
    share.restype, share.argtypes = C.c_double, [C.c_double]
    seen = {}
    for name in SETUPS:
        on = {m: wide_switch(tracer(name, m)) for m in MODES}
        survival = on["wide1"][1]
        seen[name] = survival
        has_zones = survival < 1.0
        assert on["wide0"][0] == 0 and on["a0_off"] == (0, 1.0)
        assert on["wide2"][0] == int(has_zones)
        assert on["wide1"][0] == int(has_zones and share(survival) <= 0.125), (name, survival, share(survival))
    assert wide_switch(tracer("variant5", "wide1"))[0] == 1          # the headline runs the wide pass by the rule
    assert 0.45 < seen["variant5"] < 0.52
    # the forced fall-backs: the setup with zones whose zones cover least, at the survival rate and the model's share stated above
    with_zones = {n: s for n, s in seen.items() if s < 1.0}
    print("survival rates of stage A0:", seen, "model's share for", FORCED, share(seen[FORCED]))
    assert FORCED == max(with_zones, key=with_zones.get), with_zones
    assert wide_switch(tracer(FORCED, "wide2"))[0] == 1
    assert seen[FORCED] == pytest.approx(FORCED_SURVIVAL, abs=5e-4) and share(seen[FORCED]) == pytest.approx(FORCED_SHARE, abs=2e-3)
    assert FORCED_SHARE > 5.0 * share(seen["variant5"]) and FORCED_SHARE > 0.1


@pytest.mark.parametrize("name", list(SETUPS))
def test_every_launch_size_is_the_same_for_every_knob_value(name):
    for seed in SEEDS:
        for n in RAY_COUNTS:
            ref, s = traced(tracer(name, "wide0"), (n,), seed, 0)
            assert s["N_RAYS"] == n
            for mode in MODES[1:]:
                assert_same(ref, traced(tracer(name, mode), (n,), seed, 0)[0], (name, mode, seed, n))


@pytest.mark.parametrize("name", list(SETUPS))
def test_every_offset_is_the_same_for_every_knob_value(name):
    for ray_id_offset in OFFSETS:
        for n in (257, 1025):
            ref, _ = traced(tracer(name, "wide0"), (n,), SEEDS[0], ray_id_offset)
            for mode in MODES[1:]:
                assert_same(ref, traced(tracer(name, mode), (n,), SEEDS[0], ray_id_offset)[0], (name, mode, ray_id_offset, n))


@pytest.mark.parametrize("name", list(SETUPS))
def test_one_launch_equals_three_accumulating_launches(name):
    n = 100_003
    for ray_id_offset in (0, 255):
        one, s = traced(tracer(name, "wide0"), (n,), SEEDS[1], ray_id_offset)
        assert s["N_PASSED"] > 0 or name == FORCED   # (a telescope turned by 40 degrees focuses nothing)
        for mode in MODES:
            three, _ = traced(tracer(name, mode), (1, n // 3 - 1, n - n // 3), SEEDS[1], ray_id_offset)   # cut at 1 and at N / 3
            assert_same(one, three, (name, mode, "split", ray_id_offset))


def test_f64_counters_and_sums_are_equal_to_the_last_bit():
    a, b = tracer("variant5", "wide0", "f64"), tracer("variant5", "wide2", "f64")
    for seed in SEEDS:
        for n in (65, 1025, 2_000_000):
            _, sa_ = a.trace_histogram(n, seed=seed)
            _, sb_ = b.trace_histogram(n, seed=seed)
            assert sa_["N_RAYS"] == n
            for k in sa_:
                assert np.float64(sa_[k]).tobytes() == np.float64(sb_[k]).tobytes(), (seed, n, k, sa_[k], sb_[k])
    assert sa_["N_PASSED"] > 0 and sa_["SUM_WEIGHTS"] > 0.0


def test_mass_scan_is_the_same_for_every_knob_value():
    """The fused 32-mass scan and its banded form run the same loop (mass_scan_spectra_kernel includes the same text)."""
    masses = np.linspace(0.0, 0.02, 32)
    res = {}
    for mode in MODES:
        with _environment(_env_of(mode)):
            with sa.RayTracer(make_setup("babyiaxo_xmm_gas")) as rt:
                rt.set_accumulation_mode("fixed64")
                res[mode] = [rt.trace_mass_scan(masses, n, seed=seed) for seed in SEEDS for n in (65, 1025, 100_003)]
                res[mode] += [rt.trace_mass_scan_spectra(masses, (0, 10, 8), n, seed=SEEDS[0]) for n in (257, 100_003)]
    for mode in MODES[1:]:
        for got, want in zip(res[mode], res["wide0"]):
            for d_got, d_want in zip(got, want):
                assert d_got.keys() == d_want.keys()
                for k in d_want:
                    assert np.asarray(d_got[k]).tobytes() == np.asarray(d_want[k]).tobytes(), (mode, k)
