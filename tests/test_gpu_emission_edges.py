"""The emission and opacity kernels (sart_emission.hip, sart_opacity.hip) against exact values at their edges, GPU half.

The rule, the cases and the oracle's measured error are those of tests/test_emission_reference_cpu.py (`compare` of
tests/emission_reference.py): no tolerance here comes from what the kernels return.  The kernel's own figures, measured on an
MI355X with this file (q50 / q90 / q99 / max of the relative error against the exact value; `pytest -s` prints every group):

  lattice      compton 5.0e-16 1.7e-14 1.1e-13 1.6e-13    term1 4.4e-16 1.7e-14 1.1e-13 1.6e-13
               ee_brems 4.4e-16 1.2e-15 3.0e-15 5.4e-15   free_free 5.8e-16 1.4e-15 2.9e-15 4.8e-15
               primakoff 6.8e-16 7.3e-13 1.3e-9 1.4e-7    long_plasmon 0 0 1.8e-14 1.4e-13
               trans_plasmon 2.6e-16 5.3e-14 6.2e-13 1.5e-12   iron57 0 0 0 0
  ladders      long_plasmon and trans_plasmon within a few 1e-16 of the oracle's figures on every rung (at most 2.7e-13 and
               1.9e-10); primakoff the oracle's figures digit for digit, noise included (2.7e-10 at 2^-4 ... 1.2e7 at 2^-40, q50)
  window       long_plasmon 1.2e-15 / 2.4e-15 (q50) inside, exactly zero outside
  opacity      the oracle's bits in every cell: 1.3e-16 3.3e-16 7.3e-16 8.0e-16 between the cuts (15 elements)
  no cell took the exemption of an ambiguous cut.
"""
import ctypes as C

import numpy as np
import pytest

import solaraxionraytracing_amd.emission as em
from oracle import oracle as O
from solaraxionraytracing_amd import _lib as L
from solaraxionraytracing_amd import opacity as op
from tests import emission_reference as ER
from tests.test_emission import RTOL_CLOSED_FORM, RTOL_FNEW_TERMS, RTOL_PRIMAKOFF

pytestmark = pytest.mark.gpu


def _zones(indices, all_zones=None):
    z = em.solar_zones() if all_zones is None else all_zones
    return (L.SolarZone * len(indices))(*[z[i] for i in indices])


@pytest.fixture(scope="module")
def world():
    all_zones = em.solar_zones()
    zones = _zones(ER.select_zones(all_zones), all_zones)
    params = em.default_params()
    cases = ER.build_cases(zones)
    oracle = ER.run_all(lambda z, e, a: O.emission_table(z, e, params, abs_coefs=a, components=True)[1], cases)
    kernel = ER.run_all(lambda z, e, a: em.emission_table(z, e, abs_coefs=a, params=params, components=True)[1], cases)
    return dict(all_zones=all_zones, zones=zones, params=params, cases=cases, oracle=oracle, kernel=kernel)


@pytest.mark.parametrize("run", [(name, a) for name, a, _, _ in ER.RUNS], ids=lambda r: "%s-abs%g" % r)
def test_kernel_against_exact_values(world, run):
    """Every group of the case through `compare`.  For ee_brems and free_free this is fNew recovered from the plane: the
    exact value is the mpmath prefactor times the mpmath integral, so the plane's relative error is the recovered fNew's."""
    report = []
    try:
        ER.judge_all(world["cases"], world["kernel"], world["oracle"], world["params"], report=report, only=run)
    finally:
        print("\n" + ER.format_report(report))


# ------------------------------------------------------------------------------------------------------------- totals ----

class _Ctx:
    def __enter__(self):
        self.lib, self.h = L.load_sart(), C.c_void_p()
        L.check(self.lib.sart_create(0, C.byref(self.h)))
        return self

    def __exit__(self, *exc):
        self.lib.sart_destroy(self.h)

    def table(self, zones, energies, abs_coefs=None, mask=0xFF, components=True):
        n_r, n_e = len(zones), energies.size
        p = em.default_params(terms=mask)
        out = np.full((n_r, n_e), -7.0)
        comp = np.full((8, n_r, n_e), -7.0) if components else None
        rc = self.lib.sart_emission_table(self.h, zones, n_r, L.as_dp(energies), n_e, L.as_dp(abs_coefs) if abs_coefs is not None else None,
                                          C.byref(p), L.as_dp(out), L.as_dp(comp) if components else None)
        return rc, out, comp


def test_total_is_the_ordered_sum_for_all_256_masks(world):
    zones = _zones([0, 900, 1967], world["all_zones"])
    om = ER.zone_constants(zones[2], 2)["om_pl"]
    energies = np.array([om * (1.0 + 2.0 ** -8), 0.05, 1.0, 4.2, 14.4])
    absc = np.full((3, 5), 1e-3)
    with _Ctx() as ctx:
        first = None
        for mask in range(256):
            rc, total, comp = ctx.table(zones, energies, absc, mask)
            assert rc == 0
            first = comp if first is None else first
            assert np.array_equal(comp, first)                      # all eight planes are written whatever the mask selects
            ER.check_total(total, comp, mask)
    assert all((first[k] != 0.0).any() for k in range(8))


# ------------------------------------------------------------------------------------------------------------- shapes ----

@pytest.fixture(scope="module")
def shape_reference(world):
    """3 zones x 257 energies once: held to the oracle at the suite's tolerances, then the yardstick of every smaller shape -
    a cell depends on its zone, the zone's position and its energy only, so any sub-shape must return the same bits."""
    zones = _zones([0, 900, 1967], world["all_zones"])
    energies = np.ascontiguousarray(np.exp(np.linspace(np.log(2e-3), np.log(15.0), 257)))
    absc = 1e-3 * np.exp(-energies / 3.0)[None, :] * np.array([[1.0], [0.5], [2.0]])
    with _Ctx() as ctx:
        rc, total, comp = ctx.table(zones, energies, absc)
    assert rc == 0
    _, want = O.emission_table(zones, energies, world["params"], abs_coefs=absc, components=True)
    _held_to_the_oracle(comp, want)
    return zones, energies, absc, total, comp


@pytest.mark.parametrize("n_radii", [1, 3])
@pytest.mark.parametrize("n_energies", [1, 255, 256, 257])
def test_shapes_return_the_bits_of_the_larger_table(shape_reference, n_energies, n_radii):
    zones, energies, absc, total, comp = shape_reference
    z = (L.SolarZone * n_radii)(*[zones[i] for i in range(n_radii)])
    e = np.ascontiguousarray(energies[:n_energies])
    a = np.ascontiguousarray(absc[:n_radii, :n_energies])
    with _Ctx() as ctx:
        rc, t, c = ctx.table(z, e, a)
        rc2, t2, _ = ctx.table(z, e, a, components=False)
    assert rc == 0 and rc2 == 0
    assert np.array_equal(t, total[:n_radii, :n_energies]) and np.array_equal(c, comp[:, :n_radii, :n_energies])
    assert np.array_equal(t2, t)                                    # components = None: the same total


def _held_to_the_oracle(comp, want):
    for k, name in enumerate(L.EM_TERMS):
        tol = RTOL_PRIMAKOFF if name in ("primakoff", "long_plasmon", "trans_plasmon") else (
            RTOL_FNEW_TERMS if name in ER.INTEGRAL_TERMS else RTOL_CLOSED_FORM)
        err = np.abs(comp[k] - want[k]) / np.maximum(np.abs(want[k]), np.abs(want[k]).max() * 1e-30 + 1e-300)
        assert err.max() < tol, (name, float(err.max()))


def test_the_cap_of_65535_zones_and_the_refusal_above(world):
    all_zones = world["all_zones"]
    n = 65535
    zones = (L.SolarZone * (n + 1))(*[all_zones[i % 1968] for i in range(n + 1)])
    capped = (L.SolarZone * n).from_buffer(zones)
    energies = np.array([0.2])               # inside the 18 fwhm window of the zones whose omega_pl is near
    with _Ctx() as ctx:
        rc, total, comp = ctx.table(capped, energies)
        assert rc == 0
        rc, out, cmp_out = ctx.table(zones, energies)               # 65536 zones
        assert rc == L.SART_ERR_INVALID_ARGUMENT and b"65535" in ctx.lib.sart_last_error()
        assert (out == -7.0).all() and (cmp_out == -7.0).all()      # nothing written
    assert np.isfinite(total).all() and (total > 0.0).all()
    # a zone's position decides its magnetic field (radius 0.0015 + 0.0005 R) and nothing else: the oracle at the same
    # positions, and the field-free terms of the model's second copy bit for bit those of the first
    _, want = O.emission_table(capped, energies, world["params"], components=True)
    _held_to_the_oracle(comp, want)
    for k in (0, 2, 3, 4, 7):
        assert np.array_equal(comp[k][:1968], comp[k][1968:2 * 1968]), L.EM_TERMS[k]
    assert (comp[5][:1968] != comp[5][1968:2 * 1968]).any()


def test_device_route_returns_the_host_route_bits(shape_reference):
    import torch
    zones, energies, absc, total, comp = shape_reference
    lib = L.load_sart()
    n_r, n_e = absc.shape
    d_abs = torch.from_numpy(absc).to("cuda")
    d_out = torch.full((n_r, n_e), -7.0, dtype=torch.float64, device="cuda")
    d_comp = torch.full((8, n_r, n_e), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    p = em.default_params()
    with _Ctx() as ctx:
        L.check(lib.sart_emission_table_device(ctx.h, zones, n_r, L.as_dp(energies), n_e, C.c_void_p(d_abs.data_ptr()), C.byref(p),
                                               C.c_void_p(d_out.data_ptr()), C.c_void_p(d_comp.data_ptr())))
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), total) and np.array_equal(d_comp.cpu().numpy(), comp)
        d_out.fill_(-7.0)
        torch.cuda.synchronize()
        L.check(lib.sart_emission_table_device(ctx.h, zones, n_r, L.as_dp(energies), n_e, C.c_void_p(d_abs.data_ptr()), C.byref(p),
                                               C.c_void_p(d_out.data_ptr()), None))
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), total)


# ---------------------------------------------------------------------------------------------------------- opacities ----

@pytest.mark.parametrize("n_el", [15, 1])
def test_abs_coefs_on_crafted_tables(world, n_el):
    zones = _zones([0, 1, 2], world["all_zones"])
    case = ER.OpacityCase(zones, n_el)
    struct = case.tables.as_struct(L.OpacityTables)
    want, n_outside = O.emission_abs_coefs(zones, case.n_z, case.energies, C.pointer(struct))
    got = op.abs_coefs(zones, case.n_z, case.energies, C.pointer(struct))          # raises if the kernel counts a cell off a table
    assert n_outside == 0
    cls = lambda a: np.where(np.isnan(a), 2, np.where(a == 0.0, 0, 1))
    assert np.array_equal(cls(got), cls(want)) and (got >= 0.0).all()
    assert (want == 0.0).sum() >= 4 * len(zones) and (want > 0.0).sum() >= 15 * len(zones)
    temps = [z.temp_K * 8.617e-8 for z in zones]
    nz = want != 0.0
    f = (1.0 - np.exp(-case.energies[None, :] / np.array(temps)[:, None]))[nz]
    worst = np.max(np.abs(got[nz] - want[nz]) / want[nz] * f)
    print("abs_coefs, n_elements %d: |got - want| / want * (1 - exp(-E/T)) at most %.3g; %.3f of the cells bit for bit"
          % (n_el, worst, np.mean(got == want)))
    assert worst < 4e-16
    exact, n_exact, dist = ER.abs_coef_exact(zones, case.n_z, case.energies, case.tables)
    figs = ER.compare_opacity(got, 0, exact, dist, want, n_outside, "opacity[%d]" % n_el, case.energies, temps, case.ulp_rungs)
    for name, fig in figs.items():
        print("abs_coef %s: oracle %s | kernel %s" % (name, " ".join("%.2e" % v for v in fig["oracle"]), " ".join("%.2e" % v for v in fig["got"])))


def test_abs_coefs_off_table_count(world):
    zones = _zones([0, 1, 2], world["all_zones"])
    case = ER.OpacityCase(zones, 15)
    tables, n_off = case.off_table()
    struct = tables.as_struct(L.OpacityTables)
    _, n_outside = O.emission_abs_coefs(zones, case.n_z, case.energies, C.pointer(struct))
    assert n_outside == n_off > 0
    with pytest.raises(L.SartError, match="^sart error -1: .*: %d cells evaluate a table outside" % n_off):
        op.abs_coefs(zones, case.n_z, case.energies, C.pointer(struct))
