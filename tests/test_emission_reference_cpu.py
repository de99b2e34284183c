"""The emission and opacity producers against exact values, CPU half: what the yardstick is, and that it bites.

tests/emission_reference.py evaluates readOpacityFile.nim:296-468 and :790-823 without rounding (mpmath at 50 digits,
`fractions.Fraction`).  `compare` there is the one rule this file and tests/test_gpu_emission_edges.py share:

  * per cell, the error of the kernel and of the f64 oracle (oracle/sart_emission_oracle.c) against the exact value, relative,
    with the suite's absolute floor (1e-30 of the group's largest cell; a subnormal counts as zero);
  * per group of cells - a term on the lattice, or one rung of a ladder over the 17 zones - the kernel's 50 %, 90 %, 99 %
    quantiles and its maximum may be no larger than 8 x the oracle's same figure + 4 * 2^-53 (the factor 8 is DESIGN §5's);
  * ee_brems and free_free, where the oracle's adaptive integrator is the worse side: error <= 1e-12 (1 + E/T) in every cell;
  * zero / finite non-zero / non-finite must agree with the oracle, except in cells closer to a cut than 4 * 2^-53 in
    relative terms, where either side is accepted; at most 2 cells of a case may take that exemption (the 0 and 1 ulp rungs
    of the ladders put more than two cells per zone that close by construction: the count is of exemptions taken);
  * cells with E/T > 600 are held to "zero or below the floor".

The cases (17 AGSS09 zones: every 123rd and the last): a lattice of 24 log-spaced energies in [1e-3, 15] keV plus the
energies of w = 7e-4 ... 600, with abs_coef = 1e-3 keV so that no term is identically zero; ladders E = omega_pl (1 +- 2^-k),
k = 4 ... 40, and 0, +-1, +-2 ulp of omega_pl, with abs_coef 0, 1e-6, 1e-3 and 1e3 (gamma_L >= E: the NaN-fwhm branch);
the edges of the 18 fwhm window at 1 +- 2^-20; hand-built opacity tables.  No lattice energy had to be moved away from
omega_pl: on the plain lattice at least 0.90 of the cells of every term have an oracle error <= 1e-12 (Primakoff: 0.909).

The oracle's own error against the exact values, measured here (q50 / q90 / q99 / max; `pytest -s` prints all groups):

  lattice      compton 4.1e-16 1.7e-14 1.1e-13 1.6e-13    term1 4.4e-16 1.7e-14 1.1e-13 1.6e-13
               ee_brems 2.3e-15 7.6e-15 6.4e-14 8.2e-13   free_free 2.2e-15 7.1e-15 7.9e-14 5.9e-13
               primakoff 6.8e-16 7.0e-13 1.3e-9 1.4e-7    long_plasmon 0 0 1.8e-14 1.4e-13
               trans_plasmon 2.4e-16 5.3e-14 6.2e-13 1.5e-12   iron57 0 0 0 0 (non-zero in few cells)
  ladders      long_plasmon 4e-16 ... 9e-15 (q50), at most 2.7e-13; trans_plasmon 7e-16 at 2^-4 growing to 3.6e-11 at 2^-40
               (q50) and 3e-9 at 1 ulp (abs_coef <= 1e-3), 5e-16 ... 1.5e-15 with abs_coef = 1e3
               primakoff: 2.7e-10 at 2^-4, 1.3e-4 at 2^-16, above 1 from 2^-24 on (q50)
  window       long_plasmon 1.4e-15 / 2.4e-15 (q50) inside, exactly zero outside
  opacity      between the cuts 1.3e-16 3.3e-16 7.3e-16 8.0e-16 (15 elements), 5.8e-16 2.8e-15 8.3e-15 8.3e-15 (1 element, where
               1 - exp(-E/T) is all there is); on the ulp rungs of the cuts the f64 w = E / T_table and the exact one part: T_table
               is 10^7.2 * 8.617e-8 after two roundings, and the rung 2 ulp below 20 T_table already reads w >= 20

Primakoff near omega_pl is the finding of this table: `a * 0.5 / t - 1` (:389-390) cancels completely in f64 as t and u grow,
so from E = omega_pl (1 + 2^-24) inwards the reference's own arithmetic has no correct digit.  There the rule can only
hold the kernel to the oracle's class; the formula is the reference's and stays.
"""
import numpy as np
import pytest

import solaraxionraytracing_amd.emission as em
from oracle import oracle as O
from solaraxionraytracing_amd import _lib as L
from tests import emission_reference as ER

LAT = ("lattice", ER.LATTICE_ABS)


@pytest.fixture(scope="module")
def world():
    """zones, cases, the oracle's planes and the stand-in kernel's: the oracle's, with the two integral terms formed as the
    kernel forms them (prefactor times the 80-node rule), since the oracle's adaptive integrator is not what is shipped"""
    all_zones = em.solar_zones()
    idx = ER.select_zones(all_zones)
    assert len(idx) == 17 and idx[-1] == 1967
    zones = (L.SolarZone * len(idx))(*[all_zones[i] for i in idx])
    params = em.default_params()
    cases = ER.build_cases(zones)
    oracle = ER.run_all(lambda z, e, a: O.emission_table(z, e, params, abs_coefs=a, components=True)[1], cases)
    c = cases["lattice"]
    rule = ER.rule_planes(c, params)
    return dict(zones=zones, params=params, cases=cases, oracle=oracle, rule=rule, clean=_stand_in(oracle, c, rule))


def _stand_in(oracle, c, rule, nodes=None, brems_y=None):
    w, y, y2, p2, p3 = rule
    got = {k: v.copy() for k, v in oracle.items()}
    got[LAT][2] = (p2 * ER.fnew_rule(w, y2 if brems_y is None else brems_y, nodes)).reshape(c.n_zones, -1)
    got[LAT][3] = (p3 * ER.fnew_rule(w, y, nodes)).reshape(c.n_zones, -1)
    return got


def test_fixture_lists_the_lattice_and_five_entries_recompute(world):
    w, y, y2, _, _ = world["rule"]
    assert all(ER.fnew_is_listed(a, b) and ER.fnew_is_listed(a, c) for a, b, c in zip(w, y, y2))
    for i in (0, 131, 262, 393, 543):
        for yy in (y[i], y2[i]):
            listed, fresh = ER.fnew_lookup(w[i], yy), ER.fnew_exact(w[i], yy)
            assert abs(listed / fresh - 1) < 1e-25, (w[i], yy)


def test_rule_model_against_the_exact_integral(world):
    w, y, y2, _, _ = world["rule"]
    assert w.min() < 7.1e-4 and w.max() > 599.0
    for yy in (y, y2):
        got = ER.fnew_rule(w, yy)
        worst = max(float(abs(ER._F(g) / ER.fnew_lookup(a, b) - 1)) for g, a, b in zip(got, w, yy))
        print("rule model against mpmath: worst %.3g" % worst)
        assert worst < 1e-13


def test_oracle_against_exact_and_the_clean_stand_in_passes(world):
    report = []
    ER.judge_all(world["cases"], world["clean"], world["oracle"], world["params"], report=report)
    print("\n" + ER.format_report(report))
    # the yardstick is tight where it has to be: >= 0.90 of the lattice cells of every term within 1e-12 of the exact value
    c = world["cases"]["lattice"]
    exact, z = ER.exact_for(c, world["params"], ER.LATTICE_ABS, tuple(range(8)))
    for k, name in enumerate(ER.EM_TERMS):
        vals, _ = exact[k]
        o = world["oracle"][LAT][k].ravel()
        floor = max(abs(v) for v in vals) * ER._F(ER.FLOOR)
        ok = [float(abs(ER._F(o[i]) - vals[i]) / max(abs(vals[i]), floor, ER._F(ER.DBL_MIN))) <= 1e-12
              for i in range(len(vals)) if z[i] <= ER.Z_TAIL]
        print("%-13s share of lattice cells with oracle error <= 1e-12: %.3f" % (name, np.mean(ok)))
        assert np.mean(ok) >= 0.90, name


def _planted(world, name):
    """the clean stand-in with one defect; returns (got, the run that sees it)"""
    cases, params, oracle = world["cases"], world["params"], world["oracle"]
    got = {k: v.copy() for k, v in world["clean"].items()}
    lat, lad = cases["lattice"], cases["ladder"]
    if name == "constant":
        got[LAT][0] *= 1.0 + 1e-12
        return got, LAT
    if name == "x<=1":
        om2 = np.array([[ER.zone_constants(z, R)["om_pl_sq"]] for R, z in enumerate(lad.zones)])
        hit = (lad.per_zone * lad.per_zone) / om2 == 1.0
        assert hit.sum() > 2, "the 0-ulp rung must put x == 1 in f64 in more cells than the exemption allows"
        got[("ladder", 0.0)][4][hit] = 0.0
        return got, ("ladder", 0.0)
    if name == "window":
        win = cases["window"]
        om = np.array([[ER.zone_constants(z, R)["om_pl"]] for R, z in enumerate(win.zones)])
        temp = np.array([[ER.zone_constants(z, R)["temp"]] for R, z in enumerate(win.zones)])
        got[("window", 0.0)][5][np.abs(win.per_zone - om) > 17.99 * ER.fwhm_f64(win.per_zone, temp)] = 0.0
        return got, ("window", 0.0)
    if name == "weight":
        xs, ws = ER.rule_nodes()
        ws = ws.copy()
        ws[np.argmax(ws)] *= 1.0 + 1e-10
        return _stand_in(oracle, lat, world["rule"], nodes=(xs, ws)), LAT
    if name == "panel edge":
        e = ER.RULE_EDGES
        panels = [(e[0], e[1]), (e[1], 0.31), (e[2], e[3]), (e[3], e[4]), (e[4], e[5])]
        return _stand_in(oracle, lat, world["rule"], nodes=ER.rule_nodes(panels)), LAT
    if name == "brems y":
        return _stand_in(oracle, lat, world["rule"], brems_y=world["rule"][1]), LAT
    raise KeyError(name)


@pytest.mark.parametrize("name", ["constant", "x<=1", "window", "weight", "panel edge", "brems y"])
def test_planted_defect_fails_the_rule(world, name):
    got, run = _planted(world, name)
    with pytest.raises(AssertionError) as err:
        ER.judge_all(world["cases"], got, world["oracle"], world["params"], only=run)
    print(name, "->", str(err.value)[:300])
    want = {"constant": "compton", "x<=1": "primakoff", "window": "long_plasmon", "weight": "free_free|ee_brems",
            "panel edge": "ee_brems|free_free", "brems y": "ee_brems"}[name]
    assert any(t in str(err.value) for t in want.split("|")), str(err.value)


def test_total_is_the_ordered_sum_and_a_swap_is_seen(world):
    comp = world["oracle"][LAT]
    for mask in range(256):
        ER.check_total(ER.ordered_total(comp, mask), comp, mask)
    swapped = lambda mask: (mask & ~0x50) | ((mask & 0x10) << 2) | ((mask & 0x40) >> 2)     # Primakoff and trans_plasmon swapped
    seen = 0
    for mask in range(256):
        try:
            ER.check_total(ER.ordered_total(comp, swapped(mask)), comp, mask)
        except AssertionError:
            seen += 1
    assert seen == 128                                   # every mask that selects exactly one of the two
    # and against the oracle's own total
    c = world["cases"]["lattice"]
    for mask in (0xFF, 0x51, 0x2C):
        p = em.default_params(terms=mask)
        absc = np.full((c.n_zones, c.energies.size), ER.LATTICE_ABS)
        total, full = O.emission_table(c.zones, c.energies, p, abs_coefs=absc, components=True)
        ER.check_total(total, full, mask)


# ---------------------------------------------------------------------------------------------------------- opacities ----

@pytest.fixture(scope="module")
def opacity_world():
    all_zones = em.solar_zones()
    zones = (L.SolarZone * 3)(*[all_zones[i] for i in (0, 1, 2)])
    out = {}
    for n_el in (15, 1):
        case = ER.OpacityCase(zones, n_el)
        struct = case.tables.as_struct(L.OpacityTables)
        oracle, n_out = O.emission_abs_coefs(zones, case.n_z, case.energies, C_pointer(struct))
        exact, n_exact, dist = ER.abs_coef_exact(zones, case.n_z, case.energies, case.tables)
        out[n_el] = dict(case=case, oracle=oracle, n_out=n_out, exact=exact, n_exact=n_exact, dist=dist)
    return zones, out


def C_pointer(struct):
    import ctypes as C
    return C.pointer(struct)


def _temps(zones):
    return [z.temp_K * 8.617e-8 for z in zones]


@pytest.mark.parametrize("n_el", [15, 1])
def test_opacity_oracle_against_exact(opacity_world, n_el):
    zones, world = opacity_world
    w = world[n_el]
    case, oracle = w["case"], w["oracle"]
    assert case.knots.size == 9 and w["n_out"] == 0 and w["n_exact"] <= 2
    ww = case.energies / case.temp_table
    assert np.isin(case.knots[1:], ww).all()                       # w lands on every knot in use, the first and the last
    assert (ww <= 0.0732).sum() >= 2 and (ww >= 20.0).sum() >= 2 and ((ww > 0.0732) & (ww < 20.0)).sum() >= 15
    taken = 0
    for r in range(len(zones)):
        amp = 1.0 / (1.0 - np.exp(-case.energies / _temps(zones)[r]))
        for i in range(case.energies.size):
            e, o = w["exact"][r][i], oracle[r, i]
            cls_e = 2 if ER.M.isnan(e) else (0 if e == 0 else 1)
            if cls_e != ER._cls(o):
                assert w["dist"][r, i] < ER.EPS4, (r, i, o, e, w["dist"][r, i])
                taken += 1
            elif cls_e == 1:
                assert float(abs(ER._F(o) / e - 1)) <= 2e-13 * amp[i], (r, i)
    print("n_elements %d: %d cells took the exemption, %d closer to a cut than 4 * 2^-53" % (n_el, taken, (w["dist"] < ER.EPS4).sum()))
    assert taken <= case.ulp_rungs.size * len(zones)
    figs = ER.compare_opacity(oracle, w["n_out"], w["exact"], w["dist"], oracle, w["n_out"], "opacity[%d]" % n_el, case.energies,
                              _temps(zones), case.ulp_rungs)
    for name, fig in figs.items():
        print("abs_coef %s: oracle q50 q90 q99 max: %s" % (name, " ".join("%.2e" % v for v in fig["oracle"])))
    model, n_model = ER.abs_coef_model(zones, case.n_z, case.energies, case.tables)
    assert n_model == 0 and np.array_equal(model, oracle)           # the f64 model is the oracle, bit for bit


def test_opacity_off_table_count(opacity_world):
    zones, world = opacity_world
    case = world[15]["case"]
    tables, n_off = case.off_table()
    assert n_off > 0 and n_off % len(zones) == 0
    oracle, n_out = O.emission_abs_coefs(zones, case.n_z, case.energies, C_pointer(tables.as_struct(L.OpacityTables)))
    exact, n_exact, dist = ER.abs_coef_exact(zones, case.n_z, case.energies, tables)
    assert n_out == n_off and int(np.isnan(oracle).sum()) == n_off
    # the exact count differs only by ulp rungs of the upper cut that the exact w = E / T_table puts on the other side of 20
    # (T_table in f64 is 10^7.2 * 8.617e-8 after two roundings: the -2 ulp rung sits 5.0e-16 below the cut and reads >= 20)
    off_exact = np.array([[bool(ER.M.isnan(v)) for v in row] for row in exact])
    differ = off_exact != np.isnan(oracle)
    assert n_exact == int(off_exact.sum()) and (dist[differ] < 2 * ER.EPS4).all() and np.isin(case.energies[differ.any(axis=0)], case.ulp_rungs).all()


@pytest.mark.parametrize("name", ["wrong interval", "n_outside"])
def test_planted_opacity_defect_fails_the_rule(opacity_world, name):
    zones, world = opacity_world
    w = world[15]
    case = w["case"]
    got, n = ER.abs_coef_model(zones, case.n_z, case.energies, case.tables, wrong_interval=(name == "wrong interval"))
    n += name == "n_outside"
    with pytest.raises(AssertionError):
        ER.compare_opacity(got, n, w["exact"], w["dist"], w["oracle"], w["n_out"], "opacity", case.energies, _temps(zones), case.ulp_rungs)


def test_planted_descending_sum_fails_the_rule():
    """Rounding alone tells the two orders apart only where it is made to: one zone whose heaviest metal carries the sum
    (n_Z = 2^60, opacity 1) and whose 14 lighter ones each add 0.95 * 2^-53 of it.  Ascending, the small terms gather
    before they meet the large one (error 0.7 * 2^-53); descending, each is rounded away (error 13.3 * 2^-53)."""
    all_zones = em.solar_zones()
    zones = (L.SolarZone * 1)(all_zones[0])
    tt = ER.zone_constants(zones[0], 0)["temp_table"]
    knots = [0.05, 0.08, 19.0]
    energies = np.linspace(3.0, 18.0, 40) * tt                      # E/T > 3: 1 - exp(-E/T) adds no error of its own
    tables = ER.CraftedTables(knots, [0], ER.SUMMED_ELEMENTS, [[([1.0, 2.0], [1.0, 1.0])] * 15])
    n_z = np.zeros((1, 29))
    n_z[0, list(ER.SUMMED_ELEMENTS)] = 0.95 * 2.0 ** 7
    n_z[0, 28] = 2.0 ** 60
    exact, n_exact, dist = ER.abs_coef_exact(zones, n_z, energies, tables)
    oracle, n_out = O.emission_abs_coefs(zones, n_z, energies, C_pointer(tables.as_struct(L.OpacityTables)))
    clean, _ = ER.abs_coef_model(zones, n_z, energies, tables)
    assert n_out == n_exact == 0 and np.array_equal(clean, oracle)
    ER.compare_opacity(clean, 0, exact, dist, oracle, 0, "ordering", energies, _temps(zones))
    got, _ = ER.abs_coef_model(zones, n_z, energies, tables, descending=True)
    with pytest.raises(AssertionError, match="q50"):
        ER.compare_opacity(got, 0, exact, dist, oracle, 0, "ordering", energies, _temps(zones))
