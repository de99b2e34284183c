"""Fused angular scan with per-angle images (include/sart.h: sart_trace_angular_scan_images) on the MI355X box.

performAngularScan (raytracer.nim:2778-2815) runs calculateFluxFractions at every angle and, without --noPlots, writes each angle's
focal-plane image.  Demanded here, per angle k:
  * SART_ACCUM_FIXED64: every raw slot of block k (image, scalars with both limbs, spectra) equals a sart_trace_histogram_device
    launch after sart_set_telescope_angles(NaN, a_k) on the same ray ids - bit for bit - and the scan rows equal
    sart_trace_angular_scan's;
  * the same for any split of the rays over accumulating calls or contexts (int64 sums);
  * finalized block by block, the conservation checks pass, and SART_ACCUM_F64 agrees with it to 1e-12 of the largest pixel;
  * invalid calls change nothing;
and the CLI's --angularImages writes one image CSV per angle."""
import ctypes as C
import os

import numpy as np
import pytest

import solaraxionraytracing_amd as sa
from solaraxionraytracing_amd import _lib as L
from solaraxionraytracing_amd.raytracer import angular_scan_len

from tests.conftest import make_setup
from tests.test_gpu_angular_scan import env, raw_scan

pytestmark = pytest.mark.gpu

N_IMG = 256 * 256
NRB, RMAX = 500, 10.0


def block_len(full, spectra):
    return N_IMG + L.SART_ACC_COUNT + ((2 * NRB + 3 * (full.energies.size + 1)) if spectra else 0)


def params(rt, n, seed, off, flags, spectra, accumulate):
    return rt.angular_scan_images_params(n, seed, off, flags, 256, spectra, NRB, RMAX, accumulate)


def raw_images(rt, torch, an, pieces, seed, flags, spectra):
    """(scan rows [K + 1][ASCAN_ROW], blocks [K][block length]) of raw int64, the rays [lo, hi) of every piece added in turn."""
    blen = block_len(rt.full, spectra)
    rows = torch.zeros(angular_scan_len(len(an)), dtype=torch.int64, device="cuda")
    blocks = torch.zeros(len(an) * blen, dtype=torch.int64, device="cuda")
    for lo, hi in pieces:
        rt.trace_angular_scan_images_device(params(rt, hi - lo, seed, lo, flags, spectra, True), an, rows.data_ptr(), blocks.data_ptr())
    rt.synchronize()
    return rows.cpu().numpy().reshape(len(an) + 1, L.ASCAN_ROW), blocks.cpu().numpy().reshape(len(an), blen)


def raw_single(rt, torch, a, n, seed, off, flags, spectra):
    acc = torch.zeros(block_len(rt.full, spectra), dtype=torch.int64, device="cuda")
    rt.set_telescope_angles(turned_y_deg=float(a))
    rt.trace_histogram_device(params(rt, n, seed, off, flags, spectra, False), acc.data_ptr())
    rt.synchronize()
    return acc.cpu().numpy()


def mixed_angles(k, top):
    """k angles, negative and positive, in no particular order (none of them 0: a single launch there runs the unrotated kernel)."""
    a = np.concatenate([-np.linspace(0.02, top, k // 3), np.linspace(0.02, top, k - k // 3)])
    return np.ascontiguousarray(np.random.default_rng(k).permutation(a))


CASES = {   # name -> (setup, knobs, flags, spectra)
    "babyiaxo_xmm": ("babyiaxo_xmm", {}, None, False),
    "babyiaxo_xmm_spectra": ("babyiaxo_xmm", {}, None, True),
    "turned_x": ("babyiaxo_xmm", {}, "turned_x", True),
    "generic": ("babyiaxo_xmm", {"SART_FORCE_GENERIC": "1"}, None, False),
    "gas": ("babyiaxo_xmm_gas", {}, None, True),
    "xray_test_source": ("babyiaxo_xmm_xray", {}, "own", True),
    "cast_llnl": ("cast_llnl", {}, None, True),
    "no_early_reject": ("babyiaxo_xmm", {"SART_NO_EARLY_REJECT": "1"}, None, True),
    "ignore_flags": ("babyiaxo_xmm", {}, L.CF_IGNORE_DET_WINDOW | L.CF_IGNORE_GAS_ABS | L.CF_IGNORE_REFLECTION, True),
}


def case(name):
    setup_name, knobs, flags, spectra = CASES[name]
    full = make_setup(setup_name)
    if flags == "turned_x":
        full.setup.telescope_turned_x_deg = 0.03
        flags = None
    elif flags == "own":
        flags = full.flags
    return full, knobs, flags, spectra


def assert_block_equals_single(block, single, label):
    diff = np.flatnonzero(block != single)
    assert diff.size == 0, (label, diff[:10], block[diff[:10]], single[diff[:10]])


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixed64_blocks_equal_single_launches_bit_for_bit(name):
    import torch
    full, knobs, flags, spectra = case(name)
    an = mixed_angles(35, 1.2 if name.startswith("cast") else 0.4)   # two launch groups: 18 + 17
    n, seed, off = 1_000_037, 17, 1000                                  # n not a multiple of 64, offset not of 256
    with env(**knobs):
        with sa.RayTracer(full) as rt:
            rt.set_accumulation_mode("fixed64")
            rows, blocks = raw_images(rt, torch, an, [(off, off + n)], seed, flags, spectra)
            scan = raw_scan(rt, torch, an, [(off, off + n)], seed, flags)
            y0 = rt.full.setup.telescope_turned_y_deg
            singles = [raw_single(rt, torch, a, n, seed, off, flags, spectra) for a in an]
            rt.set_telescope_angles(turned_y_deg=y0)
    assert np.array_equal(rows, scan), name                 # the scan rows: those of sart_trace_angular_scan
    for k, s in enumerate(singles):
        assert_block_equals_single(blocks[k], s, (name, k, an[k]))
    passed = blocks[:, N_IMG + L.ACC["N_PASSED"]]
    assert passed.max() > 1000 and (blocks[:, N_IMG + L.ACC["N_RAYS"]] == n).all()
    assert blocks[np.abs(an) <= 0.02, :N_IMG].any(axis=1).all(), name   # near the axis the spot is on the chip: the images are not empty


@pytest.mark.parametrize("k", [3, 32])
def test_one_launch_group_equals_single_launches(k):
    import torch
    full = make_setup("babyiaxo_xmm")
    an = np.ascontiguousarray(np.linspace(-0.3, 0.3, k) + 0.001)
    n, seed = 700_001, 3
    with sa.RayTracer(full) as rt:
        rt.set_accumulation_mode("fixed64")
        rows, blocks = raw_images(rt, torch, an, [(0, n)], seed, None, False)
        assert np.array_equal(rows, raw_scan(rt, torch, an, [(0, n)], seed))
        for j, a in enumerate(an):
            assert_block_equals_single(blocks[j], raw_single(rt, torch, a, n, seed, 0, None, False), (k, j))


@pytest.mark.parametrize("knobs", [{}, {"SART_FORCE_GENERIC": "1"}], ids=["default", "generic"])
def test_flux_and_image_scans_alternating_on_one_context_equal_fresh_contexts(knobs):
    """The two entry points share the launch path, the grid cache and the per-workgroup scratch of a context: either one first,
    more angles or fewer than the call before, every call writes what it writes alone on a fresh context."""
    import torch
    full = make_setup("babyiaxo_xmm")
    many, few = mixed_angles(35, 0.4), mixed_angles(3, 0.4)   # two launch groups (18 + 17) and one
    seed, off = 17, 1000
    calls = [   # (with images, angles, rays, spectra); the ray counts are off the 64 and 256 grids
        (False, many, 200_003, False),
        (True, few, 100_001, True),
        (False, few, 100_001, False),
        (True, many, 200_003, False),
    ]

    def run(rt, images, an, n, spectra):
        if images:
            return raw_images(rt, torch, an, [(off, off + n)], seed, None, spectra)
        return (raw_scan(rt, torch, an, [(off, off + n)], seed),)

    with env(**knobs):
        with sa.RayTracer(full) as rt:
            rt.set_accumulation_mode("fixed64")
            shared = [run(rt, *call) for call in calls]
        alone = []
        for call in calls:
            with sa.RayTracer(full) as rt:
                rt.set_accumulation_mode("fixed64")
                alone.append(run(rt, *call))
    for j, (got, want) in enumerate(zip(shared, alone)):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.dtype == np.int64 and np.array_equal(g, w), j
    assert np.array_equal(shared[1][0], shared[2][0])   # the image scan's rows are the flux-only scan's
    assert shared[0][0][:-1, L.ASCAN["N_PASSED"]].max() > 100 and shared[3][1][:, :N_IMG].any()   # (the calls traced something)


def test_angle_zero_agrees_with_the_unrotated_launch():
    """Turned x = y = 0: the single launch runs the unrotated kernel (an exact frame change where the rotation by 0 rounds)."""
    full = make_setup("babyiaxo_xmm")
    an = np.array([0.0, 0.1])
    n, seed = 1_000_000, 5
    with sa.RayTracer(full) as rt:
        imgs, summ, spec, _ = rt.trace_angular_scan_images(an, n, seed, spectra=True, n_radial_bins=NRB, radial_max=RMAX)
        img0, s0, sp0 = rt.trace_spectra(n, seed, n_radial_bins=NRB, radial_max=RMAX)
    assert np.abs(imgs[0] - img0).max() <= 1e-12 * img0.max()
    for key in ("N_PASSED", "N_PASSED_TILL_WINDOW", "N_HIT_NICKEL", "N_SHELL_SELECTED", "N_REACHED_TELESCOPE", "N_OUTSIDE_IMAGE"):
        assert abs(summ[0][key] - s0[key]) <= 2, key
    for key in ("SUM_WEIGHTS", "SUM_X", "SUM_Y", "SUM_R"):
        assert summ[0][key] == pytest.approx(s0[key], rel=1e-12), key
    assert np.abs(spec[0]["radial_weights"] - sp0["radial_weights"]).max() <= 1e-12 * sp0["radial_weights"].max()


def test_split_rays_and_two_contexts_sum_to_one_launch():
    import torch
    full = make_setup("cast_llnl")
    an = mixed_angles(20, 1.0)
    n, seed = 1_200_000, 9
    with sa.RayTracer(full) as rt:
        rt.set_accumulation_mode("fixed64")
        one = raw_images(rt, torch, an, [(0, n)], seed, None, True)
        two = raw_images(rt, torch, an, [(0, n // 2), (n // 2, n)], seed, None, True)
    with sa.RayTracer(full) as a, sa.RayTracer(full) as b:
        a.set_accumulation_mode("fixed64")
        b.set_accumulation_mode("fixed64")
        ra, ba = raw_images(a, torch, an, [(0, n // 2)], seed, None, True)
        rb, bb = raw_images(b, torch, an, [(n // 2, n)], seed, None, True)
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1])
    # ranks reduce as int64 sums; the two-limb sums then differ in representation only (hi 2^40 + lo)
    lim = 1 << L.FIXED_LIMB_BITS
    for k in range(len(an)):
        s, o = ba[k] + bb[k], one[1][k]
        assert np.array_equal(s[:N_IMG], o[:N_IMG]) and np.array_equal(s[N_IMG + L.SART_ACC_COUNT:], o[N_IMG + L.SART_ACC_COUNT:])
        for key, lo in L.ACC.items():
            if key in L.ACC_HI:
                hi = L.ACC_HI[key]
                assert int(s[N_IMG + lo]) + lim * int(s[N_IMG + hi]) == int(o[N_IMG + lo]) + lim * int(o[N_IMG + hi]), (k, key)
            elif lo not in L.ACC_HI.values():
                assert s[N_IMG + lo] == o[N_IMG + lo], (k, key)


def test_finalized_blocks_pass_the_checks_and_match_f64():
    import torch
    full = make_setup("babyiaxo_xmm")
    an = np.array([0.01, -0.015, 0.02, 0.005])   # the spot stays on the chip (the common quantum resolves its brightest pixel)
    n, seed = 100_000_000, 21   # (a pixel of n rays carries ~q sqrt(n / 12) of rounding: relative to it, larger images agree better)
    with sa.RayTracer(full) as rt:
        rt.set_accumulation_mode("fixed64")
        p = params(rt, n, seed, 0, None, True, False)
        blen = block_len(full, True)
        rows = torch.zeros(angular_scan_len(len(an)), dtype=torch.int64, device="cuda")
        blocks = torch.zeros(len(an) * blen, dtype=torch.float64, device="cuda")
        rt.trace_angular_scan_images_device(p, an, rows.data_ptr(), blocks.data_ptr())
        for k in range(len(an)):
            rt.finalize_accumulator_device(p, blocks.data_ptr() + 8 * k * blen)
        rt.synchronize()   # raises if a finalize found unresolved weights or a slot that does not add up
        fin = blocks.cpu().numpy().reshape(len(an), blen)
        imgs_fx, summ_fx, spec_fx, rows_fx = rt.trace_angular_scan_images(an, n, seed, spectra=True, n_radial_bins=NRB, radial_max=RMAX)
        rt.set_accumulation_mode("f64")
        imgs, summ, spec, rows_f = rt.trace_angular_scan_images(an, n, seed, spectra=True, n_radial_bins=NRB, radial_max=RMAX)
    for k in range(len(an)):
        assert np.array_equal(fin[k, :N_IMG].reshape(256, 256), imgs_fx[k])   # the blocking form finalizes the same way
        top = imgs[k].max()
        assert top > 0 and np.abs(imgs_fx[k] - imgs[k]).max() <= 1e-12 * top, k
        for key in ("N_PASSED", "N_PASSED_TILL_WINDOW", "N_HIT_NICKEL", "N_SHELL_SELECTED", "N_REACHED_TELESCOPE", "N_OUTSIDE_IMAGE", "N_RAYS"):
            assert summ_fx[k][key] == summ[k][key], (k, key)
        for key in ("SUM_WEIGHTS", "SUM_X", "SUM_Y", "SUM_R"):
            assert summ_fx[k][key] == pytest.approx(summ[k][key], rel=1e-11), (k, key)
        assert np.array_equal(spec_fx[k]["radial_counts"], spec[k]["radial_counts"])
        assert np.array_equal(spec_fx[k]["energy_counts"], spec[k]["energy_counts"])
        assert rows_f[0]["SUM_WEIGHTS"][k] == pytest.approx(summ[k]["SUM_WEIGHTS"], rel=1e-12)
        assert rows_fx[0]["N_PASSED"][k] == summ_fx[k]["N_PASSED"]


def test_invalid_calls_change_nothing():
    import torch
    full = make_setup("babyiaxo_xmm")
    an = np.array([0.05, 0.1, -0.02])
    n, seed = 300_000, 4
    with sa.RayTracer(full) as rt:
        rt.set_accumulation_mode("fixed64")
        fresh = rt.trace_angular_scan_images(an, n, seed)
    with sa.RayTracer(full) as rt:
        rt.set_accumulation_mode("fixed64")
        lib, h = rt.lib, rt.handle
        blen = block_len(full, False)
        rows = torch.zeros(angular_scan_len(3), dtype=torch.int64, device="cuda")
        blocks = torch.full((3 * blen,), 7, dtype=torch.int64, device="cuda")
        good = params(rt, n, seed, 0, None, False, False)
        flux_only = params(rt, n, seed, 0, None, False, False)
        flux_only.image_nx = flux_only.image_ny = 0
        half = params(rt, n, seed, 0, None, False, False)
        half.image_ny = 0
        bad_calls = [
            (flux_only, an, 3, rows.data_ptr(), blocks.data_ptr()),
            (half, an, 3, rows.data_ptr(), blocks.data_ptr()),
            (good, np.array([0.05, np.nan, 0.1]), 3, rows.data_ptr(), blocks.data_ptr()),
            (good, np.array([0.05, 90.0, 0.1]), 3, rows.data_ptr(), blocks.data_ptr()),
            (good, np.array([0.05, -91.0, np.inf]), 3, rows.data_ptr(), blocks.data_ptr()),
            (good, an, 0, rows.data_ptr(), blocks.data_ptr()),
            (good, an, 3, None, blocks.data_ptr()),
            (good, an, 3, rows.data_ptr(), None),
        ]
        for p, a, k, r, b in bad_calls:
            a = np.ascontiguousarray(a, dtype=np.float64)
            rc = lib.sart_trace_angular_scan_images_device(h, C.byref(p), L.as_dp(a), k, C.c_void_p(r), C.c_void_p(b))
            assert rc == -1, (p.image_nx, a, k)   # SART_ERR_INVALID_ARGUMENT
        a = np.ascontiguousarray(an)
        assert lib.sart_trace_angular_scan_images_device(h, None, L.as_dp(a), 3, C.c_void_p(rows.data_ptr()), C.c_void_p(blocks.data_ptr())) == -1
        assert lib.sart_trace_angular_scan_images_device(h, C.byref(good), None, 3, C.c_void_p(rows.data_ptr()), C.c_void_p(blocks.data_ptr())) == -1
        assert lib.sart_trace_angular_scan_images(h, C.byref(good), L.as_dp(a), 3, None, None) == -1
        rt.synchronize()
        assert (blocks.cpu().numpy() == 7).all() and not rows.cpu().numpy().any()   # nothing was written
        again = rt.trace_angular_scan_images(an, n, seed)
    assert np.array_equal(again[0], fresh[0])
    assert again[1] == fresh[1]
    for key in fresh[3][0]:
        assert np.array_equal(again[3][0][key], fresh[3][0][key]), key


def _read_csv(path):
    with open(path) as f:
        head = f.readline()
        vals = np.loadtxt(f, delimiter=",", usecols=2)
    return head, vals


@pytest.mark.parametrize("fused", [False, True])
def test_cli_writes_one_image_per_angle(tmp_path, fused):
    from solaraxionraytracing_amd.__main__ import main
    rays = ["--rays", "200000", "--seed", "11"]
    scan = ["--angularScanMax", "0.05", "--numAngularScanPoints", "3"] + (["--fusedAngularScan"] if fused else [])
    full_dir, plain_dir, img_dir = tmp_path / "full", tmp_path / "plain", tmp_path / "images"
    assert main(rays + ["--outpath", str(full_dir)]) == 0
    assert main(rays + scan + ["--outpath", str(plain_dir)]) == 0
    assert main(rays + scan + ["--angularImages", "--outpath", str(img_dir)]) == 0
    assert sorted(os.listdir(plain_dir)) == ["angular_scan_telescope_y.csv"]   # without the switch: what the CLI always wrote
    names = ["axion_image_IAXO_angle_%s.csv" % t for t in ("0.00", "0.03", "0.05")]
    assert sorted(os.listdir(img_dir)) == sorted(["angular_scan_telescope_y.csv"] + names)
    ref_head, ref = _read_csv(full_dir / "axion_image_IAXO.csv")
    for name in names:
        head, vals = _read_csv(img_dir / name)
        assert head == ref_head and vals.size == N_IMG
        assert sum(1 for _ in open(img_dir / name)) == 1 + N_IMG
    head = open(img_dir / "angular_scan_telescope_y.csv").readline()
    assert head == open(plain_dir / "angular_scan_telescope_y.csv").readline()
    if fused:   # angle 0 on the rays of the full run: the same image (up to the rounding of the rotation by 0, see above)
        _, a0 = _read_csv(img_dir / names[0])
        assert np.abs(a0 - ref).max() <= 1e-9 * ref.max()
        assert open(img_dir / "angular_scan_telescope_y.csv").read() != ""
    else:       # the host loop keeps NaN in the error column
        last = open(img_dir / "angular_scan_telescope_y.csv").read().splitlines()[1:]
        assert all(l.endswith(",nan") for l in last), last
