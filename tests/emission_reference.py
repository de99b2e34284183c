"""Exact references for the emission-table and absorption-coefficient producers (sart_emission.hip, sart_opacity.hip;
DESIGN §3.4), the one comparison rule the CPU and the GPU tests share, and the cases both run.

Nothing here imports the package or the oracle: the exact values come from mpmath (50 digits) and `fractions.Fraction`,
the models of what the kernels write come from numpy / `math` in f64.

"Exact" means: the formulas of readOpacityFile.nim:296-468 and :790-823 evaluated without rounding on the f64 inputs the
entry points take (the fields of `sart_solar_zone_t`, the energy, the absorption coefficient, the couplings) and on the
f64 values of the literals the sources spell (7.683e-24, 1/137, 510.998, ...); pi is pi.  Decisions (`x < 1`, the 18 fwhm
window, `omega_pl^2 > E^2`, the opacity cuts, a table's ends) are taken on those exact values, and every one reports how
far, in relative terms, the cell is from its edge.

One shortcut, stated: the integral fNew(w, y) of the two integral terms is looked up in (or integrated for) the f64
pair (w, y) as the host code rounds it, not the unrounded pair.  fNew is smooth with logarithmic derivatives of order one,
so this moves those two terms by a few 2^-53, three orders below the 1e-12 they are held to.
"""
from __future__ import annotations

import json
import math
import os
from fractions import Fraction

import mpmath
import numpy as np

M = mpmath.mp.clone()
M.dps = 50

EM_TERMS = ("compton", "term1", "ee_brems", "free_free", "primakoff", "long_plasmon", "trans_plasmon", "iron57")
TOTAL_ORDER = (0, 1, 2, 3, 6, 4, 5, 7)         # readOpacityFile.nim:849
INTEGRAL_TERMS = ("ee_brems", "free_free")
EPS4 = 4.0 * 2.0 ** -53                          # allowance of `compare`, and the width below which a cut is ambiguous
FACTOR = 8.0                                     # no further from the exact value than eight times the f64 build
INTEGRAL_YARDSTICK = 1e-12                       # test_kernel_integral_is_exact_where_the_adaptive_integrator_is_not
Z_TAIL = 600.0                                   # E/T beyond which a cell is held to "zero or below the floor"
FLOOR = 1e-30                                    # absolute floor: this share of the group's largest cell (tests/test_emission.py)
GOLDEN_FNEW = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fnew_reference.json")


def _F(x):
    """f64 -> mpf, exactly"""
    return M.mpf(float(x))


# ------------------------------------------------------------------------------------------------------------- fNew ----

def fnew_exact(w, y):
    """fNew(w, y) = int_0^inf x e^{-x^2} [I(sqrt(x^2+w)+x) - I(sqrt(x^2+w)-x)] dx, I(t) = (y^2/(t^2+y^2) + ln(t^2+y^2))/2
    (:296-326) by tanh-sinh quadrature at 50 digits, split where the integrand changes scale."""
    w, y = _F(w), _F(y)
    y2 = y * y

    def inner(t):
        q = t * t + y2
        return (y2 / q + M.log(q)) / 2

    def outer(x):
        s = M.sqrt(x * x + w)
        to = s + x
        return x * M.exp(-x * x) * (inner(to) - inner(w / to))      # sqrt(x^2+w) - x = w / (sqrt(x^2+w) + x), no cancellation

    sw = M.sqrt(w)
    pts = sorted({M.mpf(0), sw / 4, sw, y, M.mpf("0.3"), M.mpf(1), M.mpf(2), M.mpf(4), M.mpf(7), M.mpf(12)})
    return M.quad(outer, pts + [M.inf])


GL16_X = (0.0950125098376374401853193, 0.2816035507792589132304605, 0.4580167776572273863424194, 0.6178762444026437484466718,
          0.7554044083550030338951012, 0.8656312023878317438804679, 0.9445750230732325760779884, 0.9894009349916499325961542)
GL16_W = (0.1894506104550684962853967, 0.1826034150449235888667637, 0.1691565193950025381893121, 0.1495959888165767320815017,
          0.1246289712555338720524763, 0.0951585116824927848099251, 0.0622535239386478928628438, 0.0271524594117540948517806)
RULE_EDGES = (0.0, 0.05, 0.3, 1.0, 2.2, 6.0)


def rule_nodes(panels=None):
    """The kernel's 80 nodes and weights: 5 panels by 16-point Gauss-Legendre, the weights times x e^{-x^2}.
    panels: [(a, b), ...] instead of the kernel's, to plant a defect."""
    xs, ws = [], []
    for a, b in (zip(RULE_EDGES[:-1], RULE_EDGES[1:]) if panels is None else panels):
        c, h = 0.5 * (a + b), 0.5 * (b - a)
        for j in range(7, -1, -1):
            xs.append(c - h * GL16_X[j]); ws.append(h * GL16_W[j])
        for j in range(8):
            xs.append(c + h * GL16_X[j]); ws.append(h * GL16_W[j])
    xs, ws = np.array(xs), np.array(ws)
    return xs, ws * xs * np.exp(-xs * xs)


def fnew_rule(w, y, nodes=None):
    """numpy model of the kernel's fixed rule in plain f64 (the textbook form of the integrand, not the kernel's
    shared-reciprocal form): fNew for arrays w, y."""
    xs, ws = rule_nodes() if nodes is None else nodes
    w = np.asarray(w, dtype=np.float64).reshape(-1, 1)
    y2 = (np.asarray(y, dtype=np.float64) ** 2).reshape(-1, 1)
    s = np.sqrt(xs * xs + w)
    to = s + xs
    frm = w / to
    a_hi, a_lo = to * to + y2, frm * frm + y2
    g = y2 * (a_lo - a_hi) / (a_hi * a_lo) + np.log(a_hi / a_lo)
    return 0.5 * (g * ws).sum(axis=1)


_fnew_table = None


def fnew_lookup(w, y):
    """fNew at the f64 pair (w, y): from tests/golden/fnew_reference.json where it is listed, else integrated now."""
    global _fnew_table
    if _fnew_table is None:
        _fnew_table = {}
        if os.path.exists(GOLDEN_FNEW):
            with open(GOLDEN_FNEW) as f:
                for ew, ey, v in json.load(f)["entries"]:
                    _fnew_table[(ew, ey)] = v
    key = (float(w).hex(), float(y).hex())
    if key in _fnew_table:
        return M.mpf(_fnew_table[key])
    return fnew_exact(w, y)


def fnew_is_listed(w, y):
    if _fnew_table is None:
        fnew_lookup(w, y)                      # loads the fixture
    return (float(w).hex(), float(y).hex()) in _fnew_table


# --------------------------------------------------------------------------------------- the host code's zone constants ----

def zone_constants(zone, R):
    """The per-radius constants in f64 as the host code of sart_emission.hip writes them (`math`, the same expressions in the
    same order): what places the ladders and keys the fNew fixture."""
    k_alpha, k_me, k_pi = 1.0 / 137.0, 510.998, math.pi
    n_e = zone.n_e * 7.683e-24
    temp = zone.temp_K * 8.617e-8
    temp_table = math.pow(10.0, float(zone.temp_index) * 0.025) * 8.617e-8
    n_dens = n_e + zone.n_H * 7.645e-24 + 4.0 * zone.n_He * 7.645e-24
    ks2 = (4.0 * k_pi * k_alpha / temp) * n_dens
    y = math.sqrt(ks2) / math.sqrt(2.0 * k_me * temp)
    om_pl_sq = 4.0 * k_alpha * k_pi * n_e / k_me
    return dict(n_e=n_e, temp=temp, temp_table=temp_table, ks2=ks2, y=y, y_sqrt2=math.sqrt(2.0) * y, om_pl_sq=om_pl_sq,
                om_pl=math.sqrt(om_pl_sq), radius=0.0015 + float(R) * 0.0005)


def fwhm_f64(E, temp, abs_coef=0.0):
    """fwhm of longPlasmon (:427-431) in numpy f64, as the kernel writes it"""
    E = np.asarray(E, dtype=np.float64)
    gamma_l = np.maximum((1.0 - np.exp(-(E / temp))) * abs_coef, 1e-4)
    xi2 = gamma_l * E
    with np.errstate(invalid="ignore"):
        return np.sqrt(E * E + xi2) - np.sqrt(E * E - xi2)


# ---------------------------------------------------------------------------------------------------- the eight terms ----

def bfield_exact(r):
    """bfield (:328-352) at the radius r (mpf); decisions on the exact values"""
    radius_cz, size_tach, radius_outer, size_outer = _F(0.712), _F(0.02), _F(0.96), _F(0.035)
    lambda1 = _F(10.0) * radius_cz + 1
    lambda_factor = (1 + lambda1) * M.power(1 + 1 / lambda1, lambda1)
    b = M.mpf(0)
    if r < radius_cz + size_tach:
        x = (r / radius_cz) ** 2
        if x < 1:
            b = _F(3.0e3) * lambda_factor * x * M.power(1 - x, lambda1)
        yy = ((r - radius_cz) / size_tach) ** 2
        if yy < 1:
            b = _F(50.0) * (1 - yy)
    else:
        zz = ((r - radius_outer) / size_outer) ** 2
        b = _F(4.0) * (1 - zz) if zz < 1 else M.mpf(0)
    return b / (_F(1.0e6) * _F(1.4440271) * _F(1.0e-3) * M.sqrt(4 * M.pi))


def terms_exact(zone, E, abs_coef, params, R=None, want=range(8), fnew=fnew_lookup):
    """The eight terms of readOpacityFile.nim:360-468 for one cell.  `R` is the zone's position in the array the entry
    point gets (its radius for the magnetic field is 0.0015 + 0.0005 R, :751); without it the radius is zone.radius_frac.
    Returns (values[8] as mpf, None where not wanted; dist[8]: the smallest relative distance of the term's decisions from
    their edges, inf where it takes none; E / T as a float)."""
    want = set(want)
    alpha, me, amu = _F(1.0 / 137.0), _F(510.998), _F(1.6605e-24)
    E, a = _F(E), _F(abs_coef)
    g_ae, g_ag, g_an = _F(params.g_ae), _F(params.g_agamma), _F(params.g_anuclei)
    ne = _F(zone.n_e) * _F(7.683e-24)
    T = _F(zone.temp_K) * _F(8.617e-8)
    n_dens = ne + _F(zone.n_H) * _F(7.645e-24) + 4 * _F(zone.n_He) * _F(7.645e-24)
    ks2 = (4 * M.pi * alpha / T) * n_dens
    om_pl_sq = 4 * alpha * M.pi * ne / me
    rho_kev = _F(zone.rho) * _F(7.683e-24) * _F(5.60958616722e29)
    nzz2 = (_F(zone.rho) / amu) * _F(7.683e-24)
    radius = _F(zone.radius_frac) if R is None else _F(0.0015) + R * _F(0.0005)
    z = E / T
    bose, emz = M.expm1(z), M.exp(-z)
    om2 = E * E
    me35 = me ** 3 * M.sqrt(me)
    v, dist = [None] * 8, [math.inf] * 8

    if 0 in want:
        v[0] = (alpha * g_ae * g_ae * om2 * ne) / (3 * me ** 4 * bose)
    if 1 in want:
        v[1] = (g_ae * g_ae * om2 * a) / (2 * (4 * M.pi * alpha) * me * me * bose)
    if 2 in want or 3 in want:
        c = zone_constants(zone, 0 if R is None else R)
        w_f64 = float(E) / c["temp_table"]
        if 2 in want:
            v[2] = (alpha * alpha * g_ae * g_ae * 4 * M.sqrt(M.pi) * ne * ne * emz * fnew(w_f64, c["y_sqrt2"])) / \
                   (3 * M.sqrt(T) * me35 * E)
        if 3 in want:
            v[3] = (fnew(w_f64, c["y"]) * alpha * alpha * g_ae * g_ae * 8 * M.sqrt(M.pi) * ne * nzz2 * emz) / \
                   (3 * M.sqrt(2 * T) * me35 * E)
    if 4 in want:
        x = om2 / om_pl_sq
        dist[4] = float(abs(x - 1))
        if x < 1:
            v[4] = M.mpf(0)
        elif x == 1:
            v[4] = M.inf
        else:
            phase = 2 / (M.sqrt(1 - 1 / x) * bose)
            s = 2 * E * M.sqrt(om2 - om_pl_sq)
            t, u = ks2 / s, (2 * om2 - om_pl_sq) / s
            br = M.mpf(0)
            if u > 1:
                br += (u * u - 1) * M.log((u - 1) / (u + 1))
            vv = u + t
            if vv > 1:
                br -= (vv * vv - 1) * M.log((vv - 1) / (vv + 1))
            br = br * (1 / (2 * t)) - 1
            v[4] = (g_ag * g_ag * _F(1e-12) * alpha / 8) * phase * n_dens * br
    if 5 in want or 6 in want:
        bf = bfield_exact(radius)
    if 5 in want:
        gamma_l = max((1 - emz) * a, _F(1e-4))
        xi2 = gamma_l * E
        inside = True
        if xi2 > om2:
            dist[5] = float(xi2 / om2 - 1)           # fwhm is NaN in f64: the comparison is false and the cell is computed
        else:
            fwhm = M.sqrt(om2 + xi2) - M.sqrt(om2 - xi2)
            off = abs(E - M.sqrt(om_pl_sq))
            dist[5] = min(float(abs(off / (18 * fwhm) - 1)), float(1 - xi2 / om2) if xi2 != om2 else 0.0)
            inside = not (off > 18 * fwhm)
        if inside:
            fraction = E * xi2 / ((om2 - om_pl_sq) ** 2 + xi2 * xi2)
            v[5] = (g_ag * g_ag * _F(1e-12)) * (bf * bf / 3) * fraction / bose
        else:
            v[5] = M.mpf(0)
    if 6 in want:
        dist[6] = float(abs(om_pl_sq / om2 - 1))
        if om_pl_sq > om2:
            v[6] = M.mpf(0)
        else:
            gamma = (1 - emz) * a
            q = M.sqrt(1 - om_pl_sq / om2) - 1
            dp2 = om2 * q * q
            dt2 = g_ag * g_ag * _F(1e-12) * (bf * bf / 3) / 4
            den = (dp2 + (gamma / 2) ** 2) * bose
            v[6] = M.mpf(0) if gamma == 0 and den != 0 else (M.nan if den == 0 else 2 * gamma * dt2 / den)
    if 7 in want:
        tau_gamma, n = _F(1.3e-6) * _F(1.519e18), _F(3.0e17) * _F(1.7826e-30)
        e_gamma = _F(14.4)
        m_fe = _F(56.9353928) * _F(1.6605e-24) * _F(5.60958616722e29)
        eu = M.exp(-(e_gamma / T))
        w_1 = 4 * eu / (2 + 4 * eu)
        sigma = e_gamma * M.sqrt(T / m_fe)
        n_a = n * w_1 * (_F(1.82) * g_an * g_an) / tau_gamma
        v[7] = n_a * M.exp(-(E - e_gamma) ** 2 / (2 * sigma * sigma)) * rho_kev * M.sqrt(2 * M.pi) * M.pi / (sigma * om2)
    return v, dist, float(z)


def integral_prefactors(zone, E, params):
    """(brems, free-free) prefactors of fNew as mpf: term = prefactor * fNew (:364-367, :378-381)"""
    one = lambda w, y: M.mpf(1)
    v, _, _ = terms_exact(zone, E, 0.0, params, R=0, want=(2, 3), fnew=one)
    return v[2], v[3]


# ------------------------------------------------------------------------------------------------- the comparison rule ----

DBL_MIN = 2.0 ** -1022


def _cls(x):
    """0 zero, 1 finite non-zero, 2 non-finite.  A subnormal counts as zero: it has not the format's relative precision,
    and whether exp() returns one or flushes it is the maths library's choice."""
    x = float(x)
    return 2 if not math.isfinite(x) else (0 if abs(x) < DBL_MIN else 1)


def _quantiles(e):
    if len(e) == 0:
        return (0.0, 0.0, 0.0, 0.0)
    e = np.asarray(e, dtype=np.float64)
    return tuple(float(q) for q in np.quantile(e, (0.5, 0.9, 0.99))) + (float(e.max()),)


def compare(term, got, exact, oracle, group, dist=None, z=None, max_ambiguous=2):
    """The one rule (module docstring of tests/test_emission_reference_cpu.py).  `got`, `oracle`: f64 per cell; `exact`: mpf
    per cell; `dist`: the cell's decision distance (inf without one); `z`: E/T.  Raises AssertionError naming `group`;
    returns the figures: {"got": (q50, q90, q99, max), "oracle": (...), "ambiguous": cells that took the cut exemption,
    "near_cut": cells closer to a cut than 4 * 2^-53, "judged": cells that entered the quantiles}."""
    got = np.asarray(got, dtype=np.float64).ravel()
    oracle = np.asarray(oracle, dtype=np.float64).ravel()
    exact = list(exact)
    n = len(exact)
    assert got.size == n and oracle.size == n, (group, term, "shapes")
    dist = np.full(n, np.inf) if dist is None else np.asarray(dist, dtype=np.float64).ravel()
    z = np.zeros(n) if z is None else np.asarray(z, dtype=np.float64).ravel()
    finite_exact = [abs(e) for e in exact if M.isfinite(e)]
    scale = max(finite_exact) if finite_exact else M.mpf(0)
    floor = max(scale * _F(FLOOR), _F(DBL_MIN)) if scale != 0 else M.mpf(0)
    what = "%s / %s" % (group, term)
    e_got, e_orc, zs, ambiguous, problems = [], [], [], 0, []
    for i in range(n):
        if z[i] > Z_TAIL:                                  # deep tail: zero or below the floor
            if not (got[i] == 0.0 or (math.isfinite(got[i]) and abs(_F(got[i])) <= floor)):
                problems.append("cell %d: E/T = %.0f but %r is above the floor" % (i, z[i], got[i]))
            continue
        cg, co = _cls(got[i]), _cls(oracle[i])
        if cg != co:
            if dist[i] < EPS4:
                ambiguous += 1
            else:
                problems.append("cell %d: class %d, the oracle's %d (got %r, oracle %r, exact %s, cut distance %.3g)"
                                % (i, cg, co, got[i], oracle[i], M.nstr(exact[i], 8), dist[i]))
            continue
        if cg == 2 or not M.isfinite(exact[i]):
            continue
        den = max(abs(exact[i]), floor)
        if den == 0:
            if got[i] != 0.0:
                problems.append("cell %d: %r where the term is zero everywhere" % (i, got[i]))
            continue
        g_i, o_i = (0.0, 0.0) if cg == 0 else (got[i], oracle[i])          # a subnormal is judged as the zero it counts as
        e_got.append(float(abs(_F(g_i) - exact[i]) / den))
        e_orc.append(float(abs(_F(o_i) - exact[i]) / den))
        zs.append(z[i])
    qg, qo = _quantiles(e_got), _quantiles(e_orc)
    if term in INTEGRAL_TERMS:
        # the oracle's adaptive integrator is the worse side: the yardstick is 1e-12 (1 + E/T), cell by cell
        norm = np.asarray(e_got) / (1.0 + np.asarray(zs)) if e_got else np.zeros(0)
        qn = _quantiles(norm)
        if qn[3] > INTEGRAL_YARDSTICK + EPS4:
            problems.append("error / (1 + E/T): q50 %.3g q90 %.3g q99 %.3g max %.3g above 1e-12" % qn)
    else:
        for name, g, o in zip(("q50", "q90", "q99", "max"), qg, qo):
            if g > FACTOR * o + EPS4:
                problems.append("%s %.3g above 8 x %.3g + 4 * 2^-53" % (name, g, o))
    if ambiguous > max_ambiguous:
        problems.append("%d cells took the exemption of an ambiguous cut (at most %d)" % (ambiguous, max_ambiguous))
    if problems:
        raise AssertionError("%s: %s" % (what, "; ".join(problems[:6])))
    return {"got": qg, "oracle": qo, "ambiguous": ambiguous, "near_cut": int((dist < EPS4).sum()), "judged": len(e_got)}


def ordered_total(components, mask):
    """total of the selected components in the order of :849, f64 additions one after the other"""
    total = np.zeros_like(components[0])
    for k in TOTAL_ORDER:
        if mask & (1 << k):
            total = total + components[k]
    return total


def check_total(total, components, mask):
    want = ordered_total(components, mask)
    same = (total == want) | (np.isnan(total) & np.isnan(want))
    assert same.all(), "mask 0x%02x: total is not the ordered sum of its components in %d cells" % (mask, int((~same).sum()))


# ----------------------------------------------------------------------------------------------------------- the cases ----

ZONE_STRIDE = 123
W_RUNGS = (7e-4, 1e-3, 1e-2, 0.1, 1.0, 10.0, 100.0, 600.0)
LADDER_K = tuple(range(4, 41, 4))
LADDER_ULPS = (-2, -1, 0, 1, 2)
LADDER_ABS = (0.0, 1e-6, 1e-3, 1e3)


def select_zones(all_zones):
    """every 123rd zone of the model plus the last: 17 of the 1968 AGSS09 zones"""
    idx = list(range(0, len(all_zones), ZONE_STRIDE))
    if idx[-1] != len(all_zones) - 1:
        idx.append(len(all_zones) - 1)
    return idx


def _ulps(x, k):
    for _ in range(abs(k)):
        x = math.nextafter(x, math.inf if k > 0 else 0.0)
    return x


class Case:
    """Energies per zone, flattened for one call: the entry points take one energy list for all zones, so the list is the
    concatenation of the zones' own and cell (r, j) of the case is cell (r, r * n_per_zone + j) of the table."""

    def __init__(self, name, zones, per_zone, rungs):
        self.name, self.zones = name, zones
        self.per_zone = np.asarray(per_zone, dtype=np.float64)          # [n_zones][n_per_zone]
        self.rungs = list(rungs)                                        # label of column j
        self.n_zones, self.n_per_zone = self.per_zone.shape
        assert self.n_zones <= 17 and self.n_per_zone <= 64
        self.energies = np.ascontiguousarray(self.per_zone.ravel())

    def pick(self, plane):
        """[n_zones][n_zones * n_per_zone] -> the case's own cells [n_zones][n_per_zone]"""
        plane = np.asarray(plane)
        r = np.arange(self.n_zones)[:, None]
        return plane[r, r * self.n_per_zone + np.arange(self.n_per_zone)[None, :]]


def lattice_case(zones):
    base = np.exp(np.linspace(math.log(1e-3), math.log(15.0), 24))
    per_zone = [np.concatenate([base, [w * zone_constants(z, R)["temp_table"] for w in W_RUNGS]]) for R, z in enumerate(zones)]
    return Case("lattice", zones, per_zone, ["E%02d" % i for i in range(24)] + ["w=%g" % w for w in W_RUNGS])


def ladder_case(zones):
    per_zone, rungs = [], []
    for R, z in enumerate(zones):
        om = zone_constants(z, R)["om_pl"]
        row = [om * (1.0 - 2.0 ** -k) for k in LADDER_K] + [_ulps(om, u) for u in LADDER_ULPS] + [om * (1.0 + 2.0 ** -k) for k in LADDER_K]
        per_zone.append(row)
    rungs = ["-2^-%d" % k for k in LADDER_K] + ["%+dulp" % u for u in LADDER_ULPS] + ["+2^-%d" % k for k in LADDER_K]
    return Case("ladder", zones, per_zone, rungs)


def ladder_is_above(rung):
    """the rungs Primakoff is judged on: E above omega_pl, and E = fl(omega_pl) itself, where f64 may see x == 1"""
    return rung.startswith("+")


def window_case(zones):
    """E = omega_pl +- 18 fwhm(E) (1 +- 2^-20) with abs_coef = 0 (gamma_L = 1e-4), solved by fixed-point iteration in f64; a
    rung below zero energy (the outer zones, omega_pl < 18e-4 keV) is replaced by its mirror above."""
    per_zone = []
    for R, z in enumerate(zones):
        c = zone_constants(z, R)
        row = []
        for side in (-1.0, 1.0):
            for rel in (1.0 - 2.0 ** -20, 1.0 + 2.0 ** -20):
                E = c["om_pl"]
                for _ in range(60):
                    E_new = c["om_pl"] + side * 18.0 * float(fwhm_f64(max(E, 1e-300), c["temp"])) * rel
                    if not (E_new > 0.0) or not math.isfinite(E_new):
                        break
                    E = E_new
                else:
                    row.append(E)
                    continue
                row.append(None)
        up = {0: 2, 1: 3}
        row = [row[up[j]] if row[j] is None else row[j] for j in range(2)] + row[2:]
        per_zone.append(row)
    return Case("window", zones, per_zone, ["below,inside", "below,outside", "above,inside", "above,outside"])


# ---------------------------------------------------------------------------------------------------------- opacities ----

def _frac(x):
    return Fraction(float(x))


def _mpf_to_fraction(x):
    sign, man, exp, _ = x._mpf_
    f = Fraction(int(man)) * (Fraction(2) ** int(exp))
    return -f if sign else f


def _interp_exact(xs, ys, x):
    """numericalnim's Linear1D on exact numbers: (value, outside, relative distance of x from the nearer table end)"""
    x0, xn = xs[0], xs[-1]
    d = min(abs(x - x0) / abs(x0), abs(x - xn) / abs(xn)) if x0 != 0 else abs(x - xn) / abs(xn)
    if x < x0 or x > xn:
        return None, True, d
    lo, hi = 0, len(xs) - 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if xs[mid] <= x:
            lo = mid
        else:
            hi = mid
    return ys[lo] + (x - xs[lo]) * (ys[lo + 1] - ys[lo]) / (xs[lo + 1] - xs[lo]), False, d


def abs_coef_exact(zones, n_z, energies, tables):
    """readOpacityFile.nim:790-823 from a description like sart_opacity_tables_t (`CraftedTables` below, or anything with
    the same attributes as numpy arrays) in `fractions.Fraction`, the final 1 - exp(-E/T) in mpmath.
    Returns (values [n_radii][n_energies] of mpf, NaN where a table is left; n_outside; dist [n_radii][n_energies])."""
    t = tables
    u = [_frac(v) for v in t.u_mesh]
    lines = [Fraction(i) for i in range(len(u))]
    consts = _frac(1.97327e-8) * _frac(0.528e-8) * _frac(0.528e-8)
    out, dist, n_outside = [], np.full((len(zones), len(energies)), np.inf), 0
    for R, zone in enumerate(zones):
        tt = _mpf_to_fraction(M.power(10, _F(0.025) * int(zone.temp_index)) * _F(8.617e-8))
        T = _F(zone.temp_K) * _F(8.617e-8)
        slot = int(t.slot_of_zone[R])
        row = []
        for iE, E in enumerate(energies):
            w = _frac(E) / tt
            d = min(abs(w / 20 - 1), abs(w / _frac(0.0732) - 1))
            if w >= 20 or w <= _frac(0.0732):
                dist[R, iE] = float(d)
                row.append(M.mpf(0))
                continue
            table, outside, d_end = _interp_exact(u, lines, w)
            d = min(d, d_end)
            total = Fraction(0)
            for k in range(t.n_elements):
                if outside:
                    break
                cell = slot * t.n_elements + k
                n, yb, xb = int(t.table_len[cell]), int(t.table_y_begin[cell]), int(t.table_x_begin[cell])
                ys = [_frac(v) for v in t.table_y[yb:yb + n]]
                xs = [Fraction(i + 1) for i in range(n)] if xb < 0 else [_frac(v) for v in t.table_x[xb:xb + n]]
                val, off, d_end = _interp_exact(xs, ys, table)
                d = min(d, d_end)
                if off:
                    outside = True
                else:
                    total += _frac(n_z[R][int(t.element_z[k])]) * val
            dist[R, iE] = float(d)
            if outside:
                n_outside += 1
                row.append(M.nan)
            else:
                total *= consts
                row.append(M.mpf(total.numerator) / M.mpf(total.denominator) * (-M.expm1(-_F(E) / T)))
        out.append(row)
    return out, n_outside, dist


def abs_coef_model(zones, n_z, energies, tables, wrong_interval=False, descending=False):
    """f64 model of the kernel's arithmetic (same operations, same order), with two defects that can be planted: the knot
    of the neighbouring interval, and the sum over the elements from the heaviest down."""
    t = tables

    def interp(xs, ys, x):
        if not (x >= xs[0]) or not (x <= xs[-1]):
            return None
        lo, hi = 0, len(xs) - 1
        while hi - lo > 1:
            mid = (lo + hi) >> 1
            if xs[mid] <= x:
                lo = mid
            else:
                hi = mid
        if wrong_interval and len(xs) > 2:
            lo = lo + 1 if lo + 2 < len(xs) else lo - 1
        return float(ys[lo]) + (x - float(xs[lo])) * (float(ys[lo + 1]) - float(ys[lo])) / (float(xs[lo + 1]) - float(xs[lo]))

    out, n_outside = np.zeros((len(zones), len(energies))), 0
    mesh_lines = np.arange(len(t.u_mesh), dtype=np.float64)
    for R, zone in enumerate(zones):
        tt = math.pow(10.0, float(zone.temp_index) * 0.025) * 8.617e-8
        T = zone.temp_K * 8.617e-8
        slot = int(t.slot_of_zone[R])
        for iE, E in enumerate(energies):
            w = float(E) / tt
            if w >= 20.0 or w <= 0.0732:
                continue
            keep, wrong_interval = wrong_interval, False           # the mesh lookup stays right: the defect is in the tables'
            table = interp(t.u_mesh, mesh_lines, w)
            wrong_interval = keep
            ok, terms = table is not None, []
            for k in range(t.n_elements):
                if not ok:
                    break
                cell = slot * t.n_elements + k
                n, yb, xb = int(t.table_len[cell]), int(t.table_y_begin[cell]), int(t.table_x_begin[cell])
                xs = np.arange(1, n + 1, dtype=np.float64) if xb < 0 else t.table_x[xb:xb + n]
                val = interp(xs, t.table_y[yb:yb + n], table)
                if val is None:
                    ok = False
                else:
                    terms.append(float(n_z[R][int(t.element_z[k])]) * val)
            if not ok:
                n_outside += 1
                out[R, iE] = np.nan
                continue
            s = 0.0
            for v in (reversed(terms) if descending else terms):
                s = s + v
            out[R, iE] = s * 1.97327e-8 * 0.528e-8 * 0.528e-8 * (1.0 - math.exp(-float(E) / T))
    return out, n_outside


SUMMED_ELEMENTS = (6, 7, 8, 10, 11, 12, 13, 14, 16, 18, 20, 24, 25, 26, 28)     # the metals of the reference's sum (:829-834)


class CraftedTables:
    """A hand-built sart_opacity_tables_t: numpy arrays under the names of the C struct's fields."""

    def __init__(self, u_mesh, slot_of_zone, element_z, tables):
        """tables[slot][element] = (abscissae or None for the line numbers 1 .. n, opacities)"""
        self.u_mesh = np.ascontiguousarray(u_mesh, dtype=np.float64)
        self.slot_of_zone = np.ascontiguousarray(slot_of_zone, dtype=np.int32)
        self.element_z = np.ascontiguousarray(element_z, dtype=np.int32)
        self.n_mesh, self.n_slots, self.n_elements = self.u_mesh.size, len(tables), len(element_z)
        xb, yb, ln, px, py = [], [], [], [], []
        for slot in tables:
            assert len(slot) == self.n_elements
            for xs, ys in slot:
                yb.append(len(py)); py.extend(ys); ln.append(len(ys))
                if xs is None:
                    xb.append(-1)
                else:
                    assert len(xs) == len(ys)
                    xb.append(len(px)); px.extend(xs)
        self.table_y_begin = np.array(yb, dtype=np.int64)
        self.table_x_begin = np.array(xb, dtype=np.int64)
        self.table_len = np.array(ln, dtype=np.int32)
        self.table_x = np.array(px if px else [0.0], dtype=np.float64)
        self.table_y = np.array(py, dtype=np.float64)
        self.n_table_x, self.n_table_y = len(px), len(py)

    def as_struct(self, struct_type):
        """fills a ctypes sart_opacity_tables_t (the caller's type: this module imports no library); the arrays stay
        owned by self, which must outlive the struct"""
        import ctypes as C
        s = struct_type()
        for name, ctype in (("u_mesh", C.c_double), ("slot_of_zone", C.c_int32), ("element_z", C.c_int32),
                            ("table_y_begin", C.c_int64), ("table_x_begin", C.c_int64), ("table_len", C.c_int32),
                            ("table_x", C.c_double), ("table_y", C.c_double)):
            setattr(s, name, getattr(self, name).ctypes.data_as(C.POINTER(ctype)))
        s.n_mesh, s.n_slots, s.n_elements = self.n_mesh, self.n_slots, self.n_elements
        s.n_table_x, s.n_table_y = self.n_table_x, self.n_table_y
        return s


class OpacityCase:
    """Zones of one table temperature, so that one mesh places w = E / T_table on its knots for all of them.

    energies: the 0, +-1, +-2 ulp rungs of 0.0732 T_table and of 20 T_table, six energies between, and the midpoints.
    mesh (9 points): knot 0 below the lower cut (line numbers below 1 lie off the line-number tables, as in the OPCD
    files), knot 1 the smallest f64 quotient E / T_table above the cut, knot 8 the largest below the upper cut, knots 2-7
    the quotients of the six energies between: w lands on knots, on the first one in use and on the last.
    tables: per slot and element in turn the line-number table of 8 points and explicit-abscissa tables of 2, 3 and 5
    points whose abscissae are f64 values the mesh interpolation returns (1 and 8 at the ends: x lands on x = n)."""

    W_BETWEEN = (0.1, 0.3, 1.0, 2.5, 6.0, 14.0)

    def __init__(self, zones, n_elements, seed=11):
        tt = math.pow(10.0, float(zones[0].temp_index) * 0.025) * 8.617e-8
        assert all(z.temp_index == zones[0].temp_index for z in zones)
        self.zones, self.temp_table = zones, tt
        lo_rungs = [_ulps(0.0732 * tt, k) for k in LADDER_ULPS]
        hi_rungs = [_ulps(20.0 * tt, k) for k in LADDER_ULPS]
        between = [w * tt for w in self.W_BETWEEN]
        self.ulp_rungs = np.array(lo_rungs + hi_rungs)
        w_of = lambda E: E / tt
        first = min(w_of(E) for E in lo_rungs + between if w_of(E) > 0.0732)
        last = max(w_of(E) for E in hi_rungs + between if w_of(E) < 20.0)
        knots = [0.05, first] + [w_of(E) for E in between] + [last]
        assert all(b > a for a, b in zip(knots[:-1], knots[1:]))
        mids = [0.5 * (a + b) * tt for a, b in zip(knots[1:-1], knots[2:])]
        self.energies = np.array(sorted(set(lo_rungs + hi_rungs + between + mids)))
        self.knots = np.array(knots)
        rng = np.random.default_rng(seed)
        # f64 values of `table` the kernel's mesh interpolation returns at the midpoints: abscissae that x lands on
        mid_tables = [self._table_f64(E / tt) for E in mids]
        kinds = [None, [1.0, 8.0], [1.0, mid_tables[2], 8.0], [1.0, mid_tables[0], 4.0, mid_tables[5], 8.0]]
        self.element_z = SUMMED_ELEMENTS if n_elements == 15 else (26,)
        tables, turn = [], 0
        for slot in range(2):
            row = []
            for _ in range(n_elements):
                xs = kinds[(turn + slot) % 4]
                turn += 1
                row.append((xs, rng.uniform(0.05, 3.0, 8 if xs is None else len(xs))))
            tables.append(row)
        self.slot_of_zone = [r % 2 for r in range(len(zones))]
        self.tables = CraftedTables(self.knots, self.slot_of_zone, self.element_z, tables)
        self._tables_spec = tables
        self.n_z = rng.uniform(1e19, 1e23, (len(zones), 29))

    def _table_f64(self, w):
        u = self.knots
        lo = int(np.searchsorted(u, w, side="right")) - 1
        lo = min(lo, len(u) - 2)
        return float(lo) + (w - u[lo]) * (float(lo + 1) - float(lo)) / (u[lo + 1] - u[lo])

    def off_table(self):
        """The same tables under a mesh that ends at the knot of w = 6: every energy with 6 < w < 20 leaves the mesh.
        Returns (tables, the number of cells that do)."""
        w = self.energies / self.temp_table
        knots = self.knots[:7]
        n_off = int(((w > knots[-1]) & (w < 20.0)).sum()) * len(self.zones)
        return CraftedTables(knots, self.slot_of_zone, self.element_z, self._tables_spec), n_off


def compare_opacity(got, got_n_outside, exact, exact_dist, oracle, oracle_n_outside, group, energies, temps, ulp_rungs=()):
    """abs_coefs through `compare` (zero / NaN / positive are its three classes), and the count of cells off a table.  Two
    groups: the energies on and between the knots, and the ulp rungs of the two cuts - there the exact w = E / T_table and
    the f64 one may sit on different sides, and the oracle's error against the exact value says so."""
    assert got_n_outside == oracle_n_outside, "%s: %d cells off a table, the oracle counts %d" % (group, got_n_outside, oracle_n_outside)
    energies = np.asarray(energies)
    z = energies[None, :] / np.asarray(temps)[:, None]
    got, oracle = np.asarray(got), np.asarray(oracle)
    rung = np.isin(energies, np.asarray(ulp_rungs))
    out = {}
    for name, sel in (("interior", ~rung), ("ulp rungs", rung)):
        if sel.any():
            flat = [v for row in exact for v, s in zip(row, sel) if s]
            out[name] = compare("abs_coef", got[:, sel], flat, oracle[:, sel], "%s %s" % (group, name), dist=exact_dist[:, sel], z=z[:, sel])
    return out


# ------------------------------------------------------------------------------------- running and judging the cases ----

LATTICE_ABS = 1e-3     # keV, every cell of the lattice: term1 and both plasmon terms are not identically zero there
RUNS = (("lattice", LATTICE_ABS, tuple(range(8)), False),
        ("ladder", 0.0, (4, 5, 6), True), ("ladder", 1e-6, (5, 6), True), ("ladder", 1e-3, (5, 6), True), ("ladder", 1e3, (5, 6), True),
        ("window", 0.0, (5,), True))            # (case, abs_coef, judged terms, one group per rung)


def build_cases(zones):
    return {"lattice": lattice_case(zones), "ladder": ladder_case(zones), "window": window_case(zones)}


def run_all(table_fn, cases):
    """table_fn(zones, energies, abs_coefs or None) -> components [8][n_zones][n_energies].  Returns {(case, abs): [8][n_zones]
    [n_per_zone]}, the cases' own cells."""
    out = {}
    for name, a, _, _ in RUNS:
        c = cases[name]
        absc = None if a == 0.0 else np.full((c.n_zones, c.energies.size), a)
        comp = table_fn(c.zones, c.energies, absc)
        out[(name, a)] = np.stack([c.pick(comp[k]) for k in range(8)])
    return out


_exact_cache = {}


def exact_for(case, params, abs_coef, want):
    """{term: (flat list of mpf, dist)} and E/T, zone-major like Case.pick; cached per (case, abs_coef, terms)"""
    key = (case.name, abs_coef, tuple(want), params.g_ae, params.g_agamma, params.g_anuclei)
    if key not in _exact_cache:
        vals = {k: [] for k in want}
        dist = {k: [] for k in want}
        zs = []
        for R, zone in enumerate(case.zones):
            for E in case.per_zone[R]:
                v, d, z = terms_exact(zone, E, abs_coef, params, R=R, want=want)
                zs.append(z)
                for k in want:
                    vals[k].append(v[k]); dist[k].append(d[k])
        _exact_cache[key] = ({k: (vals[k], np.array(dist[k])) for k in want}, np.array(zs))
    return _exact_cache[key]


def rule_planes(case, params):
    """What the kernel's two integral terms are made of, per cell of the case: w, y, sqrt(2) y in f64 and the exact
    prefactors of fNew rounded to f64 (ee_brems, free_free)."""
    w, y, y2, p2, p3 = [], [], [], [], []
    for R, zone in enumerate(case.zones):
        c = zone_constants(zone, R)
        for E in case.per_zone[R]:
            a, b = integral_prefactors(zone, E, params)
            w.append(float(E) / c["temp_table"]); y.append(c["y"]); y2.append(c["y_sqrt2"]); p2.append(float(a)); p3.append(float(b))
    return np.array(w), np.array(y), np.array(y2), np.array(p2), np.array(p3)


def judge_all(cases, got, oracle, params, report=None, only=None):
    """`compare` on every group of every run.  got / oracle: what run_all returned.  report: a list that receives
    (group, term, figures).  only: restrict to one (case, abs_coef) run."""
    for name, a, terms, by_rung in RUNS:
        if only is not None and (name, a) != only:
            continue
        c = cases[name]
        exact, z = exact_for(c, params, a, terms)
        g, o = got[(name, a)], oracle[(name, a)]
        for k in terms:
            vals, dist = exact[k]
            if not by_rung:
                fig = compare(EM_TERMS[k], g[k].ravel(), vals, o[k].ravel(), "%s[abs=%g]" % (name, a), dist=dist, z=z)
                if report is not None:
                    report.append(("%s[abs=%g]" % (name, a), EM_TERMS[k], fig))
                continue
            ambiguous = 0
            for j, rung in enumerate(c.rungs):
                if name == "ladder" and k == 4 and not ladder_is_above(rung):
                    continue
                sel = np.arange(c.n_zones) * c.n_per_zone + j
                group = "%s[abs=%g] %s" % (name, a, rung)
                fig = compare(EM_TERMS[k], g[k][:, j], [vals[i] for i in sel], o[k][:, j], group, dist=dist[sel], z=z[sel],
                              max_ambiguous=c.n_zones)
                ambiguous += fig["ambiguous"]
                if report is not None:
                    report.append((group, EM_TERMS[k], fig))
            assert ambiguous <= 2, "%s[abs=%g] / %s: %d cells took the exemption of an ambiguous cut (at most 2)" % (
                name, a, EM_TERMS[k], ambiguous)


def format_report(report):
    lines = ["%-28s %-13s %5s  %-43s %-43s %s" % ("group", "term", "cells", "oracle q50 q90 q99 max", "got q50 q90 q99 max", "near cut")]
    for group, term, f in report:
        lines.append("%-28s %-13s %5d  %-43s %-43s %d" % (group, term, f["judged"], " ".join("%.2e" % v for v in f["oracle"]),
                                                         " ".join("%.2e" % v for v in f["got"]), f["near_cut"]))
    return "\n".join(lines)
