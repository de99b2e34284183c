"""Phase B behind the mirrors runs for the live lanes only (run on the MI355X box).

The accumulating kernels switch the lanes whose ray died at the mirrors (nickel, no-hit tests) or lies beyond the pass' valid rays
off from the gathers to the end of phase B, and hand the values of those lanes on unspecified (sart_kernels.hip, phase_b: REGION).
The record kernel keeps the flat form - every lane, every default - and is the yardstick here: a histogram launch in
SART_ACCUM_FIXED64 against the records of the same ray ids binned on the host by tests/binned_records.py (image, SART_ACC_* slots,
radial and energy spectra), slot by slot with the device-against-device envelope (EPS_DEVICE, half a quantum per ray), counts
and counters without slack.

Shapes: the smallest at which the region can go wrong - launches whose valid lanes end inside a wave (1, 63, 65, 257, 4099 rays),
one full wave (64), a last phase-B pass with fewer than 64 rays, a ray_id_offset that is no multiple of 256 - for every
instantiation the small-table setups reach: variants 5 / 0 (BabyIAXO, constant path / SART_NO_PATH_CONST), 6 / 3 (gas stage), 4
(turned telescope), 0 without zones (CAST / LLNL), the generic ones 1 / 2 (SART_FORCE_GENERIC).  Then each IGNORE flag, a launch
in which no ray survives the mirrors (every wave skips the region), and the fused mass scan's hand-over of out.gas / out.weight
through the region."""
import functools

import numpy as np
import pytest

import solaraxionraytracing_amd as sa
from solaraxionraytracing_amd import _lib as L

from tests import binned_records as B
from tests.conftest import make_setup
from tests.test_gpu_binned_records import tracer
from tests.test_gpu_mass_scan import masses, raw_scan, raw_single

pytestmark = pytest.mark.gpu

SEED = B.SEED
OFFSET = 777                                  # neither a multiple of 256 nor of 64
N_RAYS = (1, 63, 64, 65, 257, 4099)
CONTEXTS = {
    "v5_babyiaxo": ("babyiaxo_xmm", {}),
    "v0_babyiaxo_ring_path": ("babyiaxo_xmm", {"SART_NO_PATH_CONST": "1"}),
    "v6_gas": ("babyiaxo_xmm_gas", {}),
    "v3_gas_ring_path": ("babyiaxo_xmm_gas", {"SART_NO_PATH_CONST": "1"}),
    "v4_rotated": ("babyiaxo_xmm_rot", {}),
    "v0_cast_llnl": ("cast_llnl", {}),
    "v1_generic": ("babyiaxo_xmm", {"SART_FORCE_GENERIC": "1"}),
    "v1_generic_gas": ("babyiaxo_xmm_gas", {"SART_FORCE_GENERIC": "1", "SART_NO_PATH_CONST": "1"}),
    "v2_generic_rotated": ("babyiaxo_xmm_rot", {"SART_FORCE_GENERIC": "1"}),
}
IGNORE_FLAGS = {"reflection": L.CF_IGNORE_REFLECTION, "det_window": L.CF_IGNORE_DET_WINDOW, "gas_abs": L.CF_IGNORE_GAS_ABS,
                "conv_prob": L.CF_IGNORE_CONV_PROB}


@functools.lru_cache(maxsize=None)
def setup_of(name):
    return make_setup(name)


def hold_to_records(rt, full, n, offset, flags, what):
    """One FIXED64 launch with spectra against the record kernel's records of the same ray ids."""
    rec = rt.traceAxionWrapper(n, seed=SEED, ray_id_offset=offset, flags=flags)
    b = B.bin_records(rec, *B.chip(full), 2000, 10.0, full.energies, full.setup.test_active)
    img, summ, spec = rt.trace_spectra(n, seed=SEED, ray_id_offset=offset, flags=flags, n_radial_bins=2000)
    print("%s: %d rays, nickel %d, till window %d, passed %d, ambiguous %d" % (what, n, int(rec["hitNickel"].sum()),
                                                                               int(rec["passedTillWindow"].sum()), b.n_passed, b.n_ambiguous_image))
    assert b.n_ambiguous_image <= B.MAX_AMBIGUOUS and b.n_ambiguous_radial <= B.MAX_AMBIGUOUS, what
    assert summ["N_RAYS"] == n, what
    assert summ["N_HIT_NICKEL"] == int((rec["hitNickel"] != 0).sum()), what
    assert summ["N_PASSED_TILL_WINDOW"] == int((rec["passedTillWindow"] != 0).sum()), what
    B.check_histogram(b, img, summ, spec, B.EPS_DEVICE, rt.fixed_quanta(), what)
    return b


@pytest.mark.parametrize("case", sorted(CONTEXTS))
def test_histogram_equals_binned_records_at_every_launch_size(case):
    name, env = CONTEXTS[case]
    full = setup_of(name)
    with tracer(full, env) as rt:
        rt.set_accumulation_mode("fixed64")
        for n in N_RAYS:
            b = hold_to_records(rt, full, n, OFFSET, None, "%s %d rays" % (case, n))
    assert b.n_passed > 100, case                 # (the largest launch has rays on the chip)


@pytest.mark.parametrize("flag", sorted(IGNORE_FLAGS))
@pytest.mark.parametrize("name", ["babyiaxo_xmm", "babyiaxo_xmm_gas"])
def test_histogram_equals_binned_records_under_each_ignore_flag(name, flag):
    full = setup_of(name)
    with tracer(full, {}) as rt:
        rt.set_accumulation_mode("fixed64")
        for n in (65, 4099):
            b = hold_to_records(rt, full, n, OFFSET, full.flags | IGNORE_FLAGS[flag], "%s ignore %s %d rays" % (name, flag, n))
    assert b.n_passed > 100, (name, flag)


# Chosen on the CPU oracle: BabyIAXO / XMM with the telescope turned by 6 degrees, seed 9 - of the ray ids [1945, 2545) none is
# alive behind the mirrors (70 of the first 257 select a shell, 61 of those end on the nickel), so every wave of the launch skips
# the region.
NO_SURVIVOR = dict(turned_y_deg=6.0, offset=1945, n=600)


@pytest.mark.parametrize("env", [{}, {"SART_FORCE_GENERIC": "1"}], ids=["v4", "v2_generic"])
def test_a_launch_without_a_ray_behind_the_mirrors(env):
    from oracle.oracle import Oracle
    full = make_setup("babyiaxo_xmm")
    full.setup.telescope_turned_y_deg = NO_SURVIVOR["turned_y_deg"]
    n, off = NO_SURVIVOR["n"], NO_SURVIVOR["offset"]
    want = Oracle(full).trace_histogram(n, seed=SEED, ray_id_offset=off)[1]
    assert want["N_PASSED_TILL_WINDOW"] == 0 and want["N_PASSED"] == 0 and want["N_HIT_NICKEL"] > 50 and want["N_SHELL_SELECTED"] > want["N_HIT_NICKEL"]
    with tracer(full, env) as rt:
        rt.set_accumulation_mode("fixed64")
        img, summ, spec = rt.trace_spectra(n, seed=SEED, ray_id_offset=off, n_radial_bins=2000)
        b = hold_to_records(rt, full, n, off, None, "no survivor %s" % (env or "as built"))
    assert b.n_passed == 0
    assert summ["N_PASSED"] == 0 and summ["N_PASSED_TILL_WINDOW"] == 0
    assert summ["N_HIT_NICKEL"] == want["N_HIT_NICKEL"] and summ["N_SHELL_SELECTED"] == want["N_SHELL_SELECTED"]
    assert not img.any() and summ["SUM_WEIGHTS"] == 0.0 and not spec["radial_counts"].any() and not spec["energy_counts"].any()


@pytest.mark.parametrize("knobs", [{}, {"SART_NO_PATH_CONST": "1"}, {"SART_FORCE_GENERIC": "1"}], ids=["v6", "v3", "v1_generic"])
def test_fused_mass_scan_of_four_masses_equals_four_single_launches(knobs):
    """The scan kernel's phase B hands out.gas and out.weight of the live lanes through the region to the per-mass loop: the raw
    FIXED64 integers of every mass equal those of a single-mass launch on the same 4099 ray ids."""
    import torch
    full = setup_of("babyiaxo_xmm_gas")
    ms = masses(4)
    n = 4099
    with tracer(full, knobs) as rt:
        rt.set_accumulation_mode("fixed64")
        scan = raw_scan(rt, torch, ms, [(OFFSET, OFFSET + n)], SEED)
        singles = [raw_single(rt, torch, m, n, SEED, off=OFFSET) for m in ms]
    shared = scan[len(ms)]
    assert shared[L.SCAN_SHARED["N_RAYS"]] == n
    for k, s in enumerate(singles):
        for a in ("SUM_WEIGHTS", "SUM_WEIGHTS_SQ"):
            assert scan[k][L.SCAN[a]] == s[L.ACC[a]] and scan[k][L.SCAN_HI[a]] == s[L.ACC_HI[a]], (k, a)
        assert scan[k][L.SCAN["N_PASSED"]] == s[L.ACC["N_PASSED"]] > 100, k
        for key in ("N_REACHED_TELESCOPE", "N_SHELL_SELECTED", "N_HIT_NICKEL"):
            assert shared[L.SCAN_SHARED[key]] == s[L.ACC[key]], key
