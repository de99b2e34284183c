"""The blocking forms of the three fused scans on ONE context (include/sart.h: sart_trace_mass_scan, sart_trace_mass_scan_spectra,
sart_trace_energy_scan, sart_trace_angular_scan, sart_trace_angular_scan_images) on the MI355X box.

The blocking forms trace into scratch that the context keeps and that they share: it only grows, and the call before may have left
more rows, fewer, or rows of another scan in it.  Demanded here: every call of a sequence in which the point count grows, shrinks
and changes shape returns what the same call returns on a fresh context -
  * SART_ACCUM_FIXED64: the finalized doubles byte for byte;
  * SART_ACCUM_F64: the counters exactly, the sums to 1e-12 (summation order of the f64 atomics)."""
import numpy as np
import pytest

import solaraxionraytracing_amd as sa
from solaraxionraytracing_amd import _lib as L

from tests.conftest import SMALL
from tests.test_gpu_energy_scan import energies

pytestmark = pytest.mark.gpu

N_RAYS, SEED = 20_000, 29   # more than one workgroup's waves: the rings fill and drain


def setup():
    """Gas stage and X-ray test source: the one setup that the mass, the energy and the angular scan all accept."""
    return sa.initFullSetup(stage=L.SK_GAS, flags=L.CF_XRAY_TEST, **SMALL)


def calls(full):
    """(label, call(rt) -> result, per-point N_PASSED of the result, the points that pass rays) in the order they run on the shared
    context.  The points that pass rays are those of the library before the scratch was shared: every mass and energy, and the
    angles up to 0.05 degrees (the X-ray test source is a parallel beam: further off axis nothing reaches the chip)."""
    n_e = full.energies.size
    bands = (n_e - 2, 1, 3)   # the test source's energy index (n_e) lies in the last band
    m = np.linspace(0.0, 0.05, 33)
    e = energies(35)[2:]   # (its first entries, 1e-300 and 0.01 keV: window and gas transmission underflow, no ray passes)
    a = np.linspace(0.0, 0.3, 33)
    per_point = lambda r: r[0]["N_PASSED"]   # mass, energy and angular scans: (per-point dict, shared counters, ...)
    every = slice(None)
    return [
        ("mass 33", lambda rt: rt.trace_mass_scan(m, N_RAYS, SEED), per_point, every),                    # groups 32 + 1
        ("energy 3", lambda rt: rt.trace_energy_scan(e[:3], N_RAYS, SEED), per_point, every),
        ("angular 33", lambda rt: rt.trace_angular_scan(a, N_RAYS, SEED), per_point, a <= 0.05),             # 17 + 16
        ("banded 2 x 3", lambda rt: rt.trace_mass_scan_spectra(m[:2], bands, N_RAYS, SEED), per_point, every),
        ("images 2", lambda rt: rt.trace_angular_scan_images(a[:2], N_RAYS, SEED, image_n=16, spectra=True, n_radial_bins=50),
         lambda r: r[3][0]["N_PASSED"], every),
        ("energy 33", lambda rt: rt.trace_energy_scan(e, N_RAYS, SEED), per_point, every),                # 17 + 16
        ("mass 1", lambda rt: rt.trace_mass_scan(m[5:6], N_RAYS, SEED), per_point, every),
    ]


def leaves(x, path=()):
    """(path, array) of every array in a result of tuples, lists and dicts."""
    if isinstance(x, dict):
        for k, v in x.items():
            yield from leaves(v, path + (k,))
    elif isinstance(x, (tuple, list)):
        for i, v in enumerate(x):
            yield from leaves(v, path + (i,))
    elif x is not None:
        yield path, np.asarray(x, dtype=np.float64)


def is_counter(path):
    return any(isinstance(k, str) and (k.startswith("N_") or k.endswith("_counts")) for k in path)


def assert_same(got, want, mode, label):
    got, want = list(leaves(got)), list(leaves(want))
    assert [p for p, _ in got] == [p for p, _ in want], label
    for (path, g), (_, w) in zip(got, want):
        assert g.shape == w.shape, (label, path)
        if mode == "fixed64":
            assert g.tobytes() == w.tobytes(), (label, path)
        elif is_counter(path):
            assert np.array_equal(g, w), (label, path)
        else:
            assert np.allclose(g, w, rtol=1e-12, atol=0.0, equal_nan=True), (label, path, np.nanmax(np.abs(g - w)))


@pytest.fixture(scope="module")
def fresh():
    """mode -> the result of every call on a context of its own (computed once, read only)."""
    full = setup()
    out = {}
    for mode in ("fixed64", "f64"):
        out[mode] = []
        for _, call, _, _ in calls(full):
            with sa.RayTracer(full) as rt:
                rt.set_accumulation_mode(mode)
                out[mode].append(call(rt))
    return out


@pytest.mark.parametrize("mode", ["fixed64", "f64"])
def test_blocking_scans_in_turn_on_one_context_equal_fresh_contexts(mode, fresh):
    full = setup()
    seq = calls(full)
    with sa.RayTracer(full) as rt:
        rt.set_accumulation_mode(mode)
        shared = [call(rt) for _, call, _, _ in seq]
    for (label, _, n_passed, passing), got, want in zip(seq, shared, fresh[mode]):
        n = np.asarray(n_passed(got))
        print(label, "N_PASSED per point:", n.astype(np.int64).tolist())
        assert_same(got, want, mode, label)
        assert n[passing].size > 0 and (n[passing] > 0).all(), label   # (the call traced something, where it did before)
