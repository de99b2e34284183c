"""The host's two proofs behind the mirror-miss shortcut (sart_api.hip: mirror_miss_bounds_of), restated in numpy and tried on rays.

(a) A ray that is, at z = l_mirror, more than kMirrorMissEps inside the paraboloid's radius there has no root of the first mirror's
quadratic that pick_root accepts - also when the roots are moved by a few ulp.  (b) Such a ray's nickel test is true if its slope
is below the bound the host derives.  The
shell constants, the slope bound and pick_root's arithmetic follow sart_api.hip (hoist_setup) and sart_kernels.hip (pick_root,
normal_z_general, reflect, phase_b); the tables are BabyIAXO / XMM's, the slope bound is that of the full solar table (1968 radii:
the largest slopes the shortcut meets)."""
import numpy as np
import pytest

import solaraxionraytracing_amd as sa

EPS = 1e-3          # kMirrorMissEps, mm^2
N_RADII = 1968
ULP = 2.0 ** -52


@pytest.fixture(scope="module")
def geo():
    s = sa.initFullSetup(n_radii=400, n_energies=300, refl_n_angles=200, refl_n_energies=200).setup
    n = s.n_shells
    g = dict(n=n, l=s.l_mirror, r1=np.array(s.all_r1[:n]), t=np.array(s.all_thickness[:n]), beta=np.deg2rad(np.array(s.all_angles_deg[:n])))
    r_sun_max = (0.0015 + (N_RADII - 1) * 0.0005) * s.radius_sun
    g["s_max"] = (r_sun_max + s.magnet_radiusCB) / (s.distance_sun_earth + s.magnet_lengthB - r_sun_max) * (1.0 + 1e-6)
    dz1 = s.magnet_lengthColdbore - s.magnet_lengthB
    g["zcb"] = -((dz1 + s.pipe_cb_vt3_length + s.pipe_vt3_xrt_length) - dz1)
    tb, l, r1 = np.tan(g["beta"]), g["l"], g["r1"]
    r3 = -tb * l + np.sqrt(tb * l * tb * l + r1 * r1)
    e = 2.0 * r3 * tb
    g.update(tb=tb, r3=r3, e=e, m1_hb=e / 2.0, m1_cc=r3 * r3 + e * l, zhi=l * np.cos(g["beta"]), r3sq=r3 * r3, r3t=r3 * tb)
    g["num"] = np.concatenate([[0.0], r1[1:] - (r1[:-1] + g["t"][:-1])])
    # the host's per-shell conditions and j_min
    lz, s_max = l - g["zcb"], g["s_max"]
    hb_max, hb_min = r1 * s_max + g["m1_hb"], g["m1_hb"] - r1 * s_max
    S = hb_max + s_max * r1
    moved = 4.0 * 2.0 ** -46 * l * S + 2.0 ** -49 * (r1 * r1 + 2.0 * l * hb_max + (s_max * l) ** 2) + np.abs(g["m1_cc"] - 2.0 * l * g["m1_hb"] - g["r3sq"])
    a_ok = (g["zhi"] <= l) & (hb_min > 1e-3) & (EPS > 1e4 * moved)
    kappa = g["r3t"] / np.sqrt(g["r3sq"] + e * lz)
    with np.errstate(all="ignore"):
        t = np.sqrt(g["num"] ** 2 * (1.0 + 1e-6) / (lz ** 2 + g["num"] ** 2))
    m_j = kappa - t * np.sqrt((1.0 + kappa ** 2) * (1.0 + s_max ** 2))
    ok = a_ok & (g["num"] > 0.0) & (m_j >= 0.4 * s_max)
    j_min, m = n, s_max
    for j in range(n - 1, 0, -1):
        if not ok[j]:
            break
        j_min, m = j, min(m, m_j[j])
    g.update(a_ok=a_ok, j_min=j_min, lz=lz, slope_sq=float(np.nextafter(np.float32(m * m), np.float32(0.0))), m_j=m_j)
    return g


def pick_root(a, hb, c, zhi, k_ulp):
    """pick_root's two roots, each moved by k_ulp units in the last place; True where one is accepted in (0, zhi)."""
    with np.errstate(all="ignore"):
        disc = hb * hb - a * c
        sq = np.sqrt(disc)
        q = -hb - np.copysign(sq, hb)
        raq = 1.0 / (a * q)
        ra, rb = q * q * raq * (1.0 + k_ulp * ULP), c * a * raq * (1.0 + k_ulp * ULP)
        return ((ra > 0.0) & (ra < zhi)) | ((rb > 0.0) & (rb < zhi))


def flagged(g, j, X0, Y0, tsx, tsy):
    xe, ye = X0 + g["l"] * tsx, Y0 + g["l"] * tsy
    return (xe * xe + (ye * ye + EPS) < g["r3sq"][j]) & (tsx * tsx + tsy * tsy < g["slope_sq"])


def check(g, j, X0, Y0, tsx, tsy, flag):
    """No flagged ray has an accepted root (roots moved by up to 8 ulp either way); every flagged ray hits the nickel."""
    a = tsx * tsx + tsy * tsy
    hb = (X0 * tsx + Y0 * tsy) + g["m1_hb"][j]
    c = (X0 * X0 + Y0 * Y0) - g["m1_cc"][j]
    for k in (-8, -3, 0, 3, 8):
        assert not np.any(pick_root(a, hb, c, g["zhi"][j], k) & flag), k
    # phase B for a ray that missed: the normal at the input point, the reflection angle, lineHitsNickel
    zcb, lz = g["zcb"], g["lz"]
    px, py = X0 + zcb * tsx, Y0 + zcb * tsy
    rho2 = px * px + py * py
    n1z = g["r3t"][j] * rho2 / np.sqrt(rho2 * (g["e"][j] * lz + g["r3sq"][j]))
    dnw = px * tsx + py * tsy + n1z
    sin2 = dnw * dnw / ((rho2 + n1z * n1z) * (1.0 + a))
    nick = sin2 * (lz * lz + g["num"][j] ** 2) > g["num"][j] ** 2
    assert np.all(nick[flag])


def test_proved_shells(geo):
    assert np.all(geo["a_ok"][1:])                       # (a) holds for every shell of this telescope
    assert geo["j_min"] == 1                             # (b): every shell above the innermost, for slopes below the bound
    assert 0.4 * geo["s_max"] <= np.sqrt(geo["slope_sq"]) <= geo["s_max"]
    assert (geo["m_j"][1:] >= geo["s_max"]).sum() == 21  # the largest slope of a ray from the Sun alone proves the outer 21 shells
    print("j_min", geo["j_min"], "of", geo["n"], "s_max", geo["s_max"], "slope bound", np.sqrt(geo["slope_sq"]))


def test_random_rays_inside_the_slope_bound(geo):
    g, rng, n = geo, np.random.default_rng(1), 1_000_000
    j = rng.integers(g["j_min"], g["n"], n)
    lo = g["r1"][j - 1] + g["t"][j - 1]
    rho0 = lo + (g["r1"][j] - lo) * rng.random(n)
    phi, psi = 2.0 * np.pi * rng.random(n), 2.0 * np.pi * rng.random(n)
    slope = g["s_max"] * np.sqrt(rng.random(n))
    X0, Y0, tsx, tsy = rho0 * np.cos(phi), rho0 * np.sin(phi), slope * np.cos(psi), slope * np.sin(psi)
    flag = flagged(g, j, X0, Y0, tsx, tsy)
    shells_hit = np.unique(j[flag])
    print("flagged", int(flag.sum()), "of", n, "in", len(shells_hit), "of", g["n"] - g["j_min"], "proved shells")
    assert 2 * len(shells_hit) >= g["n"] - g["j_min"] and flag.sum() > 1000       # the test cannot pass empty
    check(g, j, X0, Y0, tsx, tsy, flag)


def test_rays_placed_around_the_threshold(geo):
    """Rays in the x-z plane whose squared distance from the axis at z = l_mirror is n1_r3sq - eps - d, d = +-0.5, 1, 2 eps."""
    g = geo
    js, ds = np.meshgrid(np.arange(g["j_min"], g["n"]), EPS * np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0]), indexing="ij")
    j, d = js.ravel(), ds.ravel()
    gap = g["r1"][j] - (g["r1"][j - 1] + g["t"][j - 1])
    s_in = np.maximum(0.0, g["tb"][j] - 0.9 * gap / g["l"])      # inward slope that starts the ray inside the shell's aperture
    keep = s_in < 0.95 * np.sqrt(g["slope_sq"])
    j, d, s_in = j[keep], d[keep], s_in[keep]
    assert len(np.unique(j)) >= (g["n"] - g["j_min"]) // 2
    xe = np.sqrt(g["r3sq"][j] - EPS - d)
    X0, Y0, tsx, tsy = xe + g["l"] * s_in, np.zeros_like(xe), -s_in, np.zeros_like(xe)
    assert np.all((X0 > g["r1"][j - 1] + g["t"][j - 1]) & (X0 < g["r1"][j]))
    flag = flagged(g, j, X0, Y0, tsx, tsy)
    assert np.array_equal(flag, d > 0.0)                          # 0.5 eps is far above the rounding of the construction
    check(g, j, X0, Y0, tsx, tsy, flag)
