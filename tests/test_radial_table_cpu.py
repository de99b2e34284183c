"""The radial verdict table of the solar-source histogram kernels, without a GPU: a numpy restatement of the builder and of the
lookup (tests/radial_table_model.py) against a numpy restatement of the compares, radius by radius.

Radii: every breakpoint moved by 0, +-1, +-2 and +-8 ulp, every cell edge of the look-up table moved by +-1 ulp, 0, the smallest
denormal, 1e9, NaN, and 1e6 uniform radii.  Every one must agree in code and shell."""
import numpy as np
import pytest

import solaraxionraytracing_amd as sa
from solaraxionraytracing_amd import _lib as L
from tests.radial_table_model import Geo, MARKED, TABLE_MAX, crafted_radii

_setups = {}


def setup_of(name):
    if name not in _setups:
        if name == "babyiaxo_xmm":
            full = sa.initFullSetup()
        elif name == "cast_llnl":
            full = sa.initFullSetup(L.ES_CAST, L.DK_INGRID2018, L.SK_VACUUM, L.TK_LLNL, reflectivity="gold")
        elif name == "cast_abrixas":
            full = sa.initFullSetup(L.ES_CAST, L.DK_INGRID2017, L.SK_VACUUM, L.TK_ABRIXAS)
        else:
            raise KeyError(name)
        _setups[name] = full.setup
    return _setups[name]


def sure_miss_radii(s, on, turned=False):
    """Values of the kind the host derives (sart_api.hip: shell0_miss_radius_of, mirror_miss_bounds_of): shell0_miss_radius a few mm
    below R1[0] (further below for a turned telescope: the bound follows the tilt), mirror_miss_radius R1 of a shell rounded UP to a
    float - a breakpoint a few 1e-6 mm above that shell's R1, inside its glass."""
    if not on or s.telescope_kind == L.TK_LLNL:
        return -1.0, np.inf
    r1 = np.array(s.all_r1[:s.n_shells])
    # (between the edge of the inner disc or of the XMM ring and R1[0], where the code shows)
    shell0 = r1[0] - (0.4 if s.telescope_kind == L.TK_ABRIXAS else 1.2 if turned else 0.9)
    if turned:
        return shell0, np.inf
    m = np.float32(r1[0])
    if float(m) < r1[0]:
        m = np.nextafter(m, np.float32(np.inf))
    return shell0, float(m)


CASES = [("babyiaxo_xmm", False), ("cast_llnl", False), ("cast_abrixas", False), ("babyiaxo_xmm", True)]


@pytest.mark.parametrize("knobs_on", [True, False], ids=["sure_miss_on", "sure_miss_off"])
@pytest.mark.parametrize("name,turned", CASES, ids=["babyiaxo_xmm", "cast_llnl", "cast_abrixas_off_axis", "babyiaxo_xmm_turned"])
def test_table_equals_compares(name, turned, knobs_on):
    s = setup_of(name)
    shell0, mirror = sure_miss_radii(s, knobs_on, turned)
    g = Geo(s, shell0, mirror, rotated=turned)
    table = g.build()
    assert table is not None, "the shipped telescopes get a table"
    bp, words, cells = table
    assert len(bp) <= TABLE_MAX and bp[-1] == np.inf and np.all(np.diff(bp) > 0)
    # at most one breakpoint per cell: cell 0 apart (where an unordered radial distance lands) no cell is marked
    assert np.all(cells[1:] != MARKED), np.nonzero(cells == MARKED)[0]
    assert g.lut_n <= 1024
    r = crafted_radii(g, table, 1_000_000)
    got, marked = g.by_table(table, r)
    want = g.by_compares(r)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (r[bad[:5]], got[bad[:5]], want[bad[:5]])
    assert marked.sum() < 1e-2 * r.size
    codes = np.unique(want >> 6)
    assert 0 in codes and 2 in codes
    if knobs_on and g.kind != L.TK_LLNL:
        assert 1 in codes and (turned or 3 in codes)
    # the unordered radial distance: every compare false - selected, shell lut[0] + 1, neither sure-miss code
    assert g.by_compares(np.nan)[0] == (2 << 6 | (g.lut[0] + 1)) == g.by_table(table, np.nan)[0][0]


def test_marked_cells_fall_back_to_the_compares():
    """Two breakpoints forced into one cell (a sure-miss radius a hair above the inner disc's edge, outside any glass): the builder
    marks the cell, and the lookup still agrees everywhere."""
    s = setup_of("cast_abrixas")
    g = Geo(s, shell0_miss=37.5 + 1e-4, mirror_miss=np.inf)
    table = g.build()
    assert table is not None
    cells = table[2]
    marked_cells = np.nonzero(cells == MARKED)[0]
    assert marked_cells.size == 2 and int(g.cell(37.5)) in marked_cells
    r = crafted_radii(g, table, 200_000)
    got, marked = g.by_table(table, r)
    assert np.array_equal(got, g.by_compares(r)) and marked.sum() > 0


def test_no_table_where_one_code_cannot_say_it():
    """Below shell0_miss_radius AND above mirror_miss_radius: the builder gives up, the setup runs the compares."""
    s = setup_of("babyiaxo_xmm")
    r1 = np.array(s.all_r1[:s.n_shells])
    g = Geo(s, shell0_miss=r1[1] - 0.5, mirror_miss=float(np.nextafter(np.float32(r1[0]), np.float32(np.inf))))
    assert g.build() is None
