"""Per-shell breakdown of the histogram trace (include/sart.h: sart_trace_histogram_shells_device) on the MI355X box.

Demanded here:
  * the accumulator of a shells launch equals sart_trace_histogram_device's for the same params and ray ids, raw int64 slot for slot
    in SART_ACCUM_FIXED64 (against the generic kernel variants, which the shell kernel is built on; the counters also against the
    specialised ones);
  * conservation in FIXED64, exact as integers: the sum over shells of every slot is its global counter or sum, the per-shell energy
    arrays add up to the energy spectrum;
  * per shell, the passed rays, their energy bins and their weight sums equal what sart_trace_records says about the same rays;
  * launch splits and ray-id shards give the same integers; f64 and finalized FIXED64 agree; invalid arguments change nothing;
  * --shellBreakdown end to end."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import solaraxionraytracing_amd as sa
from solaraxionraytracing_amd import _lib as L

from tests.conftest import SMALL, make_setup

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO40 = 2 ** L.FIXED_LIMB_BITS
N_RADIAL = 1000


def setup_of(name):
    if name == "babyiaxo_xmm_rot":
        full = make_setup("babyiaxo_xmm")
        full.setup.telescope_turned_x_deg, full.setup.telescope_turned_y_deg = 0.01, 0.03
        return full
    if name == "cast_llnl":   # four coatings on groups of shells
        return sa.initFullSetup(L.ES_CAST, L.DK_INGRID2018, L.SK_VACUUM, L.TK_LLNL, **SMALL)
    if name == "babyiaxo_xmm_gas":
        return sa.initFullSetup(stage=L.SK_GAS, **SMALL)
    return make_setup(name)


CASES = ["babyiaxo_xmm", "cast_llnl", "babyiaxo_xmm_gas", "babyiaxo_xmm_rot", "babyiaxo_xmm_xray"]


class Tracer:
    """A RayTracer with SART_FORCE_GENERIC set while it is created (the shell kernel is the generic histogram kernel's twin)."""

    def __init__(self, full, generic=True):
        if generic:
            os.environ["SART_FORCE_GENERIC"] = "1"
        try:
            self.rt = sa.RayTracer(full)
        finally:
            os.environ.pop("SART_FORCE_GENERIC", None)

    def __enter__(self):
        return self.rt

    def __exit__(self, *exc):
        self.rt.close()


def params(rt, n, seed, off=0, spectra=True, image_n=256, accumulate=False):
    return rt.shells_params(n, seed, off, image_n=image_n, spectra=spectra, n_radial_bins=N_RADIAL, accumulate=accumulate)


def acc_len(rt, p):
    n_img = p.image_nx * p.image_ny
    return n_img + L.SART_ACC_COUNT + ((2 * p.n_radial_bins + 3 * (rt.full.energies.size + 1)) if p.spectra else 0)


def run_shells(rt, torch, pieces, seed, spectra=True, image_n=256, dtype=None):
    """Raw accumulator and block of one accumulation over the (lo, hi) ray-id pieces."""
    dtype = dtype or torch.int64
    p0 = params(rt, 1, seed, spectra=spectra, image_n=image_n)
    acc = torch.zeros(acc_len(rt, p0), dtype=dtype, device="cuda")
    blk = torch.zeros(rt.shell_block_len(spectra), dtype=dtype, device="cuda")
    for lo, hi in pieces:
        p = params(rt, hi - lo, seed, lo, spectra, image_n, accumulate=True)
        rt.trace_shells_device(p, acc.data_ptr(), blk.data_ptr())
    rt.synchronize()
    return acc.cpu().numpy(), blk.cpu().numpy()


def run_hist(rt, torch, n, seed, off=0, spectra=True, image_n=256):
    p = params(rt, n, seed, off, spectra, image_n)
    acc = torch.zeros(acc_len(rt, p), dtype=torch.int64, device="cuda")
    rt.trace_histogram_device(p, acc.data_ptr())
    rt.synchronize()
    return acc.cpu().numpy()


def split(rt, blk, spectra=True):
    ns, ne = rt.full.setup.n_shells, rt.full.energies.size
    rows = blk[:ns * L.SHELL_ROW].reshape(ns, L.SHELL_ROW)
    tail = blk[ns * L.SHELL_ROW:].reshape(2, ns, ne + 1) if spectra else None
    return rows, tail


def limbs(lo, hi):
    return int(hi) * TWO40 + int(lo)


@pytest.mark.parametrize("name", CASES)
def test_fixed64_accumulator_equals_the_histogram_and_conserves(name):
    import torch
    full = setup_of(name)
    n, seed = 400_000, 7
    with Tracer(full) as rt:
        rt.set_accumulation_mode("fixed64")
        for spectra, image_n in ((True, 256), (False, 0)):
            ref = run_hist(rt, torch, n, seed, 13, spectra, image_n)
            acc, blk = run_shells(rt, torch, [(13, 13 + n)], seed, spectra, image_n)
            np.testing.assert_array_equal(acc, ref)
            n_img = image_n * image_n
            sc = acc[n_img:n_img + L.SART_ACC_COUNT]
            rows, tail = split(rt, blk, spectra)
            assert sc[L.ACC["N_PASSED"]] > 100
            for key, gkey in (("N_SELECTED", "N_SHELL_SELECTED"), ("N_HIT_NICKEL", "N_HIT_NICKEL"),
                              ("N_PASSED_TILL_WINDOW", "N_PASSED_TILL_WINDOW"), ("N_PASSED", "N_PASSED")):
                assert int(rows[:, L.SHELL[key]].sum()) == int(sc[L.ACC[gkey]]), key
            for key in ("SUM_WEIGHTS", "SUM_WEIGHTS_SQ"):
                tot = sum(limbs(r[L.SHELL[key]], r[L.SHELL_HI[key]]) for r in rows)
                assert tot == limbs(sc[L.ACC[key]], sc[L.ACC_HI[key]]), key
                assert np.all(rows[:, L.SHELL[key]] >= 0) and np.all(rows[:, L.SHELL[key]] < TWO40)
            sel, nic = rows[:, L.SHELL["N_SELECTED"]], rows[:, L.SHELL["N_HIT_NICKEL"]]
            till, pas = rows[:, L.SHELL["N_PASSED_TILL_WINDOW"]], rows[:, L.SHELL["N_PASSED"]]
            assert np.all(sel >= nic + till) and np.all(till >= pas)
            if spectra:
                ne1 = rt.full.energies.size + 1
                en = acc[n_img + L.SART_ACC_COUNT + 2 * N_RADIAL:]
                np.testing.assert_array_equal(tail[0].sum(axis=0), en[:ne1])
                np.testing.assert_array_equal(tail[1].sum(axis=0), en[ne1:2 * ne1])
                np.testing.assert_array_equal(tail[0].sum(axis=1), pas)


@pytest.mark.parametrize("name", ["babyiaxo_xmm", "cast_llnl"])
def test_counters_equal_the_specialised_histogram(name):
    """Against the solar-source specialisations (no SART_FORCE_GENERIC): the same rays, so the same counters."""
    full = setup_of(name)
    with Tracer(full, generic=False) as rt:
        _, s_h = rt.trace_histogram(1_000_000, seed=3, ray_id_offset=1)
        _, s_s, _, shells = rt.trace_shells(1_000_000, seed=3, ray_id_offset=1)
    for k in ("N_RAYS", "N_REACHED_TELESCOPE", "N_SHELL_SELECTED", "N_HIT_NICKEL", "N_PASSED_TILL_WINDOW", "N_PASSED", "N_OUTSIDE_IMAGE"):
        assert s_h[k] == s_s[k], k
    assert s_s["SUM_WEIGHTS"] == pytest.approx(s_h["SUM_WEIGHTS"], rel=1e-12)
    assert shells["N_SELECTED"].sum() == s_s["N_SHELL_SELECTED"]
    assert shells["SUM_WEIGHTS"].sum() == pytest.approx(s_s["SUM_WEIGHTS"], rel=1e-12)


@pytest.mark.parametrize("name", ["babyiaxo_xmm", "cast_llnl", "babyiaxo_xmm_xray"])
def test_per_shell_passed_energies_and_weights_equal_the_records(name):
    import torch
    full = setup_of(name)
    n, seed, off = 300_000, 19, 512
    with Tracer(full) as rt:
        rt.set_accumulation_mode("fixed64")
        _, blk = run_shells(rt, torch, [(off, off + n)], seed)
        q = rt.fixed_quanta()["weight"]
        rec = rt.traceAxionWrapper(n, seed=seed, ray_id_offset=off)
    rows, tail = split(rt, blk)
    ns, ne = full.setup.n_shells, full.energies.size
    passed = rec[rec["passed"] == 1]
    sh = passed["shellNumber"].astype(np.int64)
    assert passed.size > 100 and sh.min() >= 0 and sh.max() < ns
    np.testing.assert_array_equal(rows[:, L.SHELL["N_PASSED"]], np.bincount(sh, minlength=ns))
    # the energy index of a record: the X-ray test source's energy is index n_energies, else the table entry it was drawn at
    e_idx = np.full(passed.size, ne) if full.setup.test_active else np.searchsorted(full.energies, passed["energiesAx"])
    cnt = np.zeros((ns, ne + 1), dtype=np.int64)
    np.add.at(cnt, (sh, e_idx), 1)
    np.testing.assert_array_equal(tail[0], cnt)
    w_fx = np.rint(passed["weights"] / q).astype(np.int64)   # to_fixed: round to nearest even of w 2^k
    want = np.zeros(ns, dtype=object)
    for s, w in zip(sh, w_fx):
        want[s] += int(w)
    got = [limbs(r[L.SHELL["SUM_WEIGHTS"]], r[L.SHELL_HI["SUM_WEIGHTS"]]) for r in rows]
    assert got == list(want)
    # a record's shellNumber is written for the rays that reach the chip only: every passed ray is one of them, and passed the window
    assert np.all(np.bincount(sh, minlength=ns) <= rows[:, L.SHELL["N_PASSED_TILL_WINDOW"]])


@pytest.mark.parametrize("name", ["babyiaxo_xmm_gas", "babyiaxo_xmm_rot"])
def test_splits_and_shards_give_the_same_integers(name):
    import torch
    full = setup_of(name)
    n, seed = 300_000, 5
    with Tracer(full) as rt:
        rt.set_accumulation_mode("fixed64")
        a1, b1 = run_shells(rt, torch, [(0, n)], seed)
        a2, b2 = run_shells(rt, torch, [(0, 77_777), (77_777, n)], seed)
        a3, b3 = run_shells(rt, torch, [(0, 123_456)], seed)
        a4, b4 = run_shells(rt, torch, [(123_456, n)], seed)
    np.testing.assert_array_equal(a1, a2)
    np.testing.assert_array_equal(b1, b2)
    # shards summed as int64 (what an all-reduce of the raw buffers does); the limbs are renormalised by value, not slot for slot
    rows1, t1 = split(rt, b1)
    rows34, t34 = split(rt, b3 + b4)
    np.testing.assert_array_equal(t1, t34)
    for j in range(4):
        np.testing.assert_array_equal(rows1[:, j], rows34[:, j])
    for key in ("SUM_WEIGHTS", "SUM_WEIGHTS_SQ"):
        for r1, r2 in zip(rows1, rows34):
            assert limbs(r1[L.SHELL[key]], r1[L.SHELL_HI[key]]) == limbs(r2[L.SHELL[key]], r2[L.SHELL_HI[key]])


@pytest.mark.parametrize("name", ["babyiaxo_xmm", "cast_llnl", "babyiaxo_xmm_xray"])
def test_f64_and_finalized_fixed64_agree(name):
    full = setup_of(name)
    with Tracer(full) as rt:
        img_f, s_f, sp_f, sh_f = rt.trace_shells(2_000_000, seed=9)
        rt.set_accumulation_mode("fixed64")
        img_x, s_x, sp_x, sh_x = rt.trace_shells(2_000_000, seed=9)
        q = rt.fixed_quanta()["weight"]
    # FIXED64 rounds every ray's weight to its quantum (<= q / 2 each): a bin of k rays agrees to k q / 2 in absolute terms
    for key in ("N_SELECTED", "N_HIT_NICKEL", "N_PASSED_TILL_WINDOW", "N_PASSED"):
        np.testing.assert_array_equal(sh_f[key], sh_x[key])
    np.testing.assert_array_equal(sh_f["energy_counts"], sh_x["energy_counts"])
    for key in ("SUM_WEIGHTS", "SUM_WEIGHTS_SQ"):
        np.testing.assert_allclose(sh_x[key], sh_f[key], rtol=1e-11, atol=1e-12 * sh_f[key].max())
    np.testing.assert_allclose(sh_x["energy_weights"], sh_f["energy_weights"], rtol=1e-11, atol=0.5 * q * sh_f["energy_counts"].max())
    assert s_x["SUM_WEIGHTS"] == pytest.approx(s_f["SUM_WEIGHTS"], rel=1e-12)
    assert sh_f["SUM_WEIGHTS"].sum() == pytest.approx(s_f["SUM_WEIGHTS"], rel=1e-12)


def test_invalid_arguments_leave_the_context_unchanged():
    import torch
    full = setup_of("babyiaxo_xmm")
    with Tracer(full) as rt:
        rt.set_accumulation_mode("fixed64")
        s0 = L.Setup()
        L.check(rt.lib.sart_get_setup(rt.handle, C.byref(s0)))
        a0, b0 = run_shells(rt, torch, [(0, 200_000)], 4)
        acc = torch.zeros(a0.size, dtype=torch.int64, device="cuda")
        blk = torch.zeros(b0.size, dtype=torch.int64, device="cuda")
        good = params(rt, 200_000, 4)
        bad = []
        for field, value in (("image_nx", -1), ("image_nx", 0), ("n_radial_bins", 0), ("radial_max", 0.0), ("image_x_max", -1.0)):
            p = params(rt, 200_000, 4)
            setattr(p, field, value)
            bad.append(p)
        for p in bad:
            with pytest.raises(L.SartError) as e:
                rt.trace_shells_device(p, acc.data_ptr(), blk.data_ptr())
            assert e.value.code == L.SART_ERR_INVALID_ARGUMENT
        for a, b in ((0, blk.data_ptr()), (acc.data_ptr(), 0)):
            assert rt.lib.sart_trace_histogram_shells_device(rt.handle, C.byref(good), C.c_void_p(a), C.c_void_p(b)) == L.SART_ERR_INVALID_ARGUMENT
        assert rt.lib.sart_finalize_shells_device(rt.handle, C.byref(good), None, C.c_void_p(blk.data_ptr())) == L.SART_ERR_INVALID_ARGUMENT
        s1 = L.Setup()
        L.check(rt.lib.sart_get_setup(rt.handle, C.byref(s1)))
        assert bytes(s0) == bytes(s1)
        a1, b1 = run_shells(rt, torch, [(0, 200_000)], 4)
    np.testing.assert_array_equal(a0, a1)
    np.testing.assert_array_equal(b0, b1)


def test_cli_shell_breakdown_end_to_end(tmp_path):
    out_a, out_b = tmp_path / "a", tmp_path / "b"
    run = lambda out, extra: subprocess.run([sys.executable, "-m", "solaraxionraytracing_amd", "--rays", "400000", "--outpath", str(out)] + extra,
                                            capture_output=True, text=True, timeout=600, cwd=ROOT)
    ra, rb = run(out_a, ["--shellBreakdown"]), run(out_b, [])
    assert ra.returncode == 0, ra.stderr[-2000:]
    assert rb.returncode == 0, rb.stderr[-2000:]
    total = float([l for l in ra.stdout.splitlines() if l.startswith("The total flux")][0].split()[-1])
    n_passed = int([l for l in ra.stdout.splitlines() if l.startswith("Passed axions ")][0].split()[-1])
    tab = sa.raytracer.read_shell_breakdown_csv(str(out_a / "shell_breakdown_IAXO.csv"))
    assert tab["flux"].sum() == pytest.approx(total, rel=1e-12)
    assert int(tab["passed"].sum()) == n_passed
    assert tab["flux fraction"].sum() == pytest.approx(1.0, rel=1e-12)
    eb = np.loadtxt(out_a / "energies_by_shell_IAXO.csv", delimiter=",", skiprows=1, ndmin=2)
    assert int(eb[:, 3].sum()) == n_passed and eb[:, 4].sum() == pytest.approx(total, rel=1e-12)
    ia = np.loadtxt(out_a / "axion_image_IAXO.csv", delimiter=",", skiprows=1, usecols=2)
    ib = np.loadtxt(out_b / "axion_image_IAXO.csv", delimiter=",", skiprows=1, usecols=2)
    np.testing.assert_allclose(ia, ib, rtol=1e-9, atol=np.abs(ib).max() * 1e-12)
