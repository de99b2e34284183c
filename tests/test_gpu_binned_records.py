"""Histogram output = records, binned on the host (run on the MI355X box).

The record path is held ray by ray to the binary128 oracle (tests/test_gpu_parity.py: identical flags, positions below 1e-10 mm,
weights to rtol 2e-8).  Here the fused histogram kernels are held, slot by slot, to those records binned by tests/binned_records.py:
every pixel, the count and weight outside the image, every radial bin, every energy index, energy_reflect and the scalars.  The
other "bit for bit the plain launch" tests of the suite (tile / no tile, shells, per-angle blocks, splits and shards) hang on this.

Envelope (tests/binned_records.py): a ray within DELTA_MM = 1e-9 mm of a slot's edge may be on either side; weights to eps = 2e-8
against the oracle's records, 1e-12 against the device's own; half a quantum per ray in SART_ACCUM_FIXED64, the summation term in
f64; counts are integers without slack; an empty slot reads exactly 0.

Conditions of every case, asserted beside the check (and printed with the FIXED64 quantum of the context): at most 2 ambiguous
rays, and at least 0.90 of the rays inside the image heavier than twice the envelope of their own pixel (moving one of those must
fail; rays outside the image are held by N_OUTSIDE_IMAGE, see binned_records.Binned.detectable_shares).  The cases are defined in
tests/binned_records.py, and tests/test_binned_records_cpu.py holds each of them to both conditions without a GPU; measured there
with the binary128 oracle, seed 9, f64 / FIXED64 with a weight bound of 16 x the heaviest ray:
  ids [0, 40 000) and [777, 40 780), 256 x 256 over the chip, 2000 and 10 000 radial bins over 10 mm, 64 bins up to the median
  pointdataR: 0 ambiguous rays in all six setups; shares babyiaxo_xmm 0.988 / 0.942, babyiaxo_xmm_gas 0.988 / 0.934, cast_llnl
  0.942 / 0.923, cast_abrixas 0.994 / 0.990, babyiaxo_xmm_rot 1.0 / 1.0, babyiaxo_xmm_xray 1.0 / 1.0;
  the six windows, FIXED64: 0 ambiguous rays; shares babyiaxo_xmm 0.942, 1.0, 0.976, 0.939, 0.976, 1.0 and cast_llnl 0.998, 1.0
  (no ray inside), 0.924, 0.914, 0.932, 1.0 (straddling, outside, small, unequal steps, y slice, one pixel); of ALL passed rays,
  the rays outside weighed against the slot "outside": 0.88 - 0.94 and 0.77 - 0.91."""
import functools
import os

import numpy as np
import pytest

import solaraxionraytracing_amd as sa

from tests import binned_records as B
from tests.conftest import make_setup

pytestmark = pytest.mark.gpu

SEED, RANGES, SETUPS = B.SEED, B.RANGES, B.SETUPS
CONTEXTS = ({}, {"SART_FORCE_GENERIC": "1"}, {"SART_NO_IMAGE_TILE": "1"})
FLAGS = ("passed", "passedTillWindow", "hitNickel", "shellNumber", "kinds", "kindsWindow")


@functools.lru_cache(maxsize=None)
def setup_of(name):
    return make_setup(name)


@functools.lru_cache(maxsize=None)
def oracle_records(name, n, offset):
    """The reference, computed once per (setup, id range) and shared: the binary128 oracle's records, read-only."""
    from oracle.oracle import Oracle
    rec = Oracle(setup_of(name), "q").trace_records(n, seed=SEED, ray_id_offset=offset)
    rec.setflags(write=False)
    return rec


def tracer(full, env):
    """A RayTracer created with the SART_* knobs of `env` set (they are read when a context is created)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return sa.RayTracer(full)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def binned(full, rec, window=None, n_bins=2000, radial_max=10.0):
    return B.bin_records(rec, *(window or B.chip(full)), n_bins, radial_max, full.energies, full.setup.test_active)


def assert_flags_equal(rt, name, n, offset):
    """What the project already guarantees: every decision of the record kernel is the oracle's."""
    rec, ref = rt.traceAxionWrapper(n, seed=SEED, ray_id_offset=offset), oracle_records(name, n, offset)
    for f in FLAGS:
        np.testing.assert_array_equal(rec[f], ref[f], err_msg=f)


def check(b, out, eps, quanta, what, spectra=False, min_share=B.MIN_DETECTABLE):
    """The two conditions of the case, then every slot."""
    img, summ = out[0], out[1]
    share, share_passed = b.detectable_shares(eps, quanta)
    print("%s: passed %d, ambiguous image %d radial %d, detectable share %.4f (of all passed rays %.4f)%s"
          % (what, b.n_passed, b.n_ambiguous_image, b.n_ambiguous_radial, share, share_passed,
             "" if quanta is None else ", weight quantum %.3e" % quanta["weight"]))
    assert b.n_ambiguous_image <= B.MAX_AMBIGUOUS, what
    assert not spectra or b.n_ambiguous_radial <= B.MAX_AMBIGUOUS, what
    assert share >= min_share, (what, share)
    B.check_histogram(b, img, summ, out[2] if spectra else None, eps, quanta, what)


def modes(rt):
    """(name, quanta getter) of the two accumulation modes; the quanta are frozen by the first launch, so they are read after it."""
    for mode in ("fixed64", "f64"):
        rt.set_accumulation_mode(mode)
        yield mode, (rt.fixed_quanta if mode == "fixed64" else lambda: None)


@pytest.mark.parametrize("name", SETUPS)
def test_image_scalars_and_outside_count(name):
    full = setup_of(name)
    refs = [(n, off, binned(full, oracle_records(name, n, off))) for n, off in RANGES]
    assert all(b.n_passed > 5000 for _, _, b in refs)
    for env in CONTEXTS:
        with tracer(full, env) as rt:
            if not env:
                for n, off in RANGES:
                    assert_flags_equal(rt, name, n, off)
            for mode, quanta in modes(rt):
                for n, off, b in refs:
                    img, summ = rt.trace_histogram(n, seed=SEED, ray_id_offset=off)
                    assert summ["N_RAYS"] == n
                    check(b, (img, summ), B.EPS_ORACLE, quanta(), "%s %s %s ids [%d, %d)" % (name, env or "as built", mode, off, off + n))


@pytest.mark.parametrize("name", B.WINDOW_SETUPS)
def test_image_windows(name):
    full = setup_of(name)
    n, off = RANGES[0]
    rec = oracle_records(name, n, off)
    with tracer(full, {}) as rt:
        rt.set_accumulation_mode("fixed64")
        for what, nx, ny, xr, yr in B.windows(full, *B.centroid(rec)):
            b = binned(full, rec, (nx, ny, xr, yr))
            out = rt.trace_image(n, nx, ny, x_range=xr, y_range=yr, seed=SEED, ray_id_offset=off)
            n_out = b.outside[0].count[0]
            if what != "unequal steps":
                assert 0 < n_out <= b.n_passed, (what, n_out)     # the window cuts the spot, or sees stray rays (if any) only
            check(b, out, B.EPS_ORACLE, rt.fixed_quanta(), "%s window %s" % (name, what))


@pytest.mark.parametrize("name", B.SPECTRA_SETUPS)
def test_spectra(name):
    full = setup_of(name)
    n, off = RANGES[1]
    rec = oracle_records(name, n, off)
    with tracer(full, {}) as rt:
        for mode, quanta in modes(rt):
            for n_bins, radial_max in B.radial_cases(rec):
                b = binned(full, rec, None, n_bins, radial_max)
                if radial_max < 10.0:
                    assert 0.4 * b.n_passed < b.radial[0].count[-1] < 0.6 * b.n_passed
                if full.setup.test_active:
                    assert b.energy[0].count[-1] == b.n_passed       # every ray of the X-ray test source: index n_energies
                out = rt.trace_spectra(n, seed=SEED, ray_id_offset=off, n_radial_bins=n_bins, radial_max=radial_max)
                check(b, out, B.EPS_ORACLE, quanta(), "%s %s spectra %d bins over %g mm" % (name, mode, n_bins, radial_max), spectra=True)


@pytest.mark.parametrize("name", ["babyiaxo_xmm_gas", "cast_abrixas"])
def test_accumulate_over_two_id_ranges(name):
    full = setup_of(name)
    n, off = RANGES[1]
    b = binned(full, oracle_records(name, n, off))
    first = 12_345
    with tracer(full, {}) as rt:
        for mode, quanta in modes(rt):
            rt.trace_spectra(first, seed=SEED, ray_id_offset=off, n_radial_bins=2000)
            out = rt.trace_spectra(n - first, seed=SEED, ray_id_offset=off + first, n_radial_bins=2000, accumulate=True)
            assert out[1]["N_RAYS"] == n
            check(b, out, B.EPS_ORACLE, quanta(), "%s %s accumulate" % (name, mode), spectra=True)


@pytest.mark.parametrize("name", ["babyiaxo_xmm", "cast_llnl"])
def test_against_the_devices_own_records(name):
    """400 000 rays, the record kernel's records of the same ids as reference, eps = 1e-12: pixels hold many rays here, and a
    difference between the record kernel's instantiation and a histogram instantiation would show.  Under SART_FORCE_GENERIC in
    FIXED64 the per-pixel quanta equal sum rint(w / quantum) of the records exactly."""
    full = setup_of(name)
    n = 400_000
    with tracer(full, {}) as rt:
        rec = rt.traceAxionWrapper(n, seed=SEED)
    b = binned(full, rec)
    assert b.n_passed > 50_000
    for env in CONTEXTS:
        with tracer(full, env) as rt:
            for mode, quanta in modes(rt):
                out = rt.trace_spectra(n, seed=SEED, n_radial_bins=2000)
                check(b, out, B.EPS_DEVICE, quanta(), "%s %s %s device records" % (name, env or "as built", mode), spectra=True)
                if mode == "fixed64" and "SART_FORCE_GENERIC" in env:
                    q = quanta()["weight"]
                    want = np.zeros(256 * 256 + 1, dtype=np.int64)
                    np.add.at(want, b.pixel_of_ray, np.rint(b.w / q).astype(np.int64))
                    got = out[0].ravel() / q
                    assert np.all(got < 2.0 ** 53) and np.array_equal(got, np.rint(got))      # finalized doubles hold the integers
                    settled = b.image[1].count == 0                                           # (no ambiguous ray at the pixel)
                    np.testing.assert_array_equal(got.astype(np.int64)[settled], want[:-1][settled])
