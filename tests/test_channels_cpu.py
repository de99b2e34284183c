"""CPU side of the emission-channel breakdown (include/sart.h: sart_trace_histogram_channels_device): the C-ABI tables, the Nim
binding, the code object of channel_histogram_kernel, the helpers that name and recombine a block, the term -> coupling map against
the CPU oracle, and the command line's new switch."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import solaraxionraytracing_amd.emission as em
from solaraxionraytracing_amd import _lib as L
from solaraxionraytracing_amd import raytracer as R
from solaraxionraytracing_amd import tables
from solaraxionraytracing_amd.__main__ import build_parser, check_channels_config, check_scan_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
NEW = ("sart_set_source_channels", "sart_set_source_channels_device", "sart_get_source_channels", "sart_clear_source_channels",
       "sart_channel_block_len", "sart_trace_histogram_channels_device", "sart_trace_histogram_channels", "sart_finalize_channels_device")


def test_entry_points_are_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sart.h")).read(), flags=re.S)
    nim = open(os.path.join(ROOT, "integration", "sart_ffi.nim")).read()
    lib = L.load_sart()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in L.SART_SYMBOLS, name
        assert re.search(r"proc %s\*" % name, nim), name
        assert hasattr(lib, name), name
    assert lib.sart_abi_version() == 5


def test_layout_constants_agree_across_header_library_and_python():
    hdr = open(os.path.join(ROOT, "include", "sart.h")).read()
    for key, slot in list(L.CHAN.items()) + [(k + "_HI", v) for k, v in L.CHAN_HI.items()]:
        assert re.search(r"SART_CHAN_%s = %d\b" % (key, slot), hdr), key
    assert re.search(r"SART_CHAN_ROW = %d\b" % L.CHAN_ROW, hdr)
    assert re.search(r"#define SART_MAX_CHANNELS %d\b" % L.MAX_CHANNELS, hdr)
    assert sorted(list(L.CHAN.values()) + list(L.CHAN_HI.values()) + [L.CHAN_RESERVED]) == list(range(L.CHAN_ROW))
    lib = L.load_sart()
    for t, ne, sp, nx, ny in ((1, 300, 0, 0, 0), (1, 300, 1, 256, 256), (3, 300, 1, 0, 0), (8, 1500, 1, 256, 256), (8, 1, 0, 7, 3),
                              (6, 300, 1, 64, 32), (0, 5, 1, 4, 4)):
        want = t * 8 + sp * t * (ne + 1) + t * nx * ny
        assert lib.sart_channel_block_len(t, ne, sp, nx, ny) == L.channel_block_len(t, ne, sp, nx, ny) == want
        assert R.channel_block_len(t, ne, bool(sp), nx, ny) == want


def _kernel_blocks(tmp_path):
    obj = tmp_path / "sart_kernels.o"
    shutil.copy(os.path.join(ROOT, "solaraxionraytracing_amd", "csrc", "build", "sart_kernels.o"), obj)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", str(obj)], check=True, capture_output=True, cwd=tmp_path)
    dev = [f for f in os.listdir(tmp_path) if "amdgcn" in f]
    assert len(dev) == 1, dev
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(tmp_path / dev[0])], capture_output=True, text=True,
                           check=True).stdout
    out = []
    for k in re.split(r"\n  - \.a", notes):
        m = re.search(r"\.name:\s+(\S+)", k)
        if m and "channel_histogram_kernel" in m.group(1):
            out.append((m.group(1), k))
    return out


def test_channel_kernel_instantiations_meet_the_ray_kernel_budgets(tmp_path):
    """Exactly {not rotated, rotated} x {f64, FIXED64}, named without `trace_`; no scratch, no spills, <= 128 VGPRs (four waves per
    SIMD at 1024 threads), LDS within 160 KB, kernel arguments within 4 KB."""
    blocks = _kernel_blocks(tmp_path)
    want = {"_ZN4sart24channel_histogram_kernelILi1024ELb%dELb%dEEEvNS_4HotAEPKNS_7DevBlobENS_9TraceArgsEPdNS_4HotBENS_11ChannelArgsE" % (r, f)
            for r in (0, 1) for f in (0, 1)}
    assert {n for n, _ in blocks} == want
    for name, k in blocks:
        assert "trace_" not in name
        g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, k).group(1))
        assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0, name
        assert g("vgpr_count") <= 128, (name, g("vgpr_count"))
        assert g("group_segment_fixed_size") <= 160 * 1024, (name, g("group_segment_fixed_size"))
        assert g("kernarg_segment_size") <= 4096, name


def _synthetic_block(t, ne, spectra, nx, ny):
    rng = np.random.default_rng(5)
    blk = np.zeros(L.channel_block_len(t, ne, spectra, nx, ny))
    rows = blk[:t * L.CHAN_ROW].reshape(t, L.CHAN_ROW)
    rows[:, L.CHAN["SUM_WEIGHTS"]] = rng.random(t) + 0.1
    rows[:, L.CHAN["SUM_WEIGHTS_SQ"]] = rng.random(t) ** 2
    rows[:, L.CHAN["N_CONTRIBUTING"]] = rng.integers(1, 100, t)
    o = t * L.CHAN_ROW
    if spectra:
        en = blk[o:o + t * (ne + 1)].reshape(t, ne + 1)
        en[:, 2] = rows[:, L.CHAN["SUM_WEIGHTS"]]
        o += t * (ne + 1)
    if nx:
        img = blk[o:].reshape(t, ny, nx)
        img[:, 1, 2] = 0.75 * rows[:, L.CHAN["SUM_WEIGHTS"]]
        rows[:, L.CHAN["SUM_WEIGHTS_OUTSIDE"]] = 0.25 * rows[:, L.CHAN["SUM_WEIGHTS"]]
    else:
        rows[:, L.CHAN["SUM_WEIGHTS_OUTSIDE"]] = rows[:, L.CHAN["SUM_WEIGHTS"]]
    return blk


@pytest.mark.parametrize("spectra,n_img", [(True, 8), (False, 8), (True, 0)])
def test_split_channels_and_the_csv_writers_round_trip(tmp_path, spectra, n_img):
    t, ne = 3, 6
    blk = _synthetic_block(t, ne, spectra, n_img, n_img)
    ch = L.split_channels(blk, t, ne, spectra, n_img, n_img)
    assert set(ch) == set(L.CHAN) | ({"energy_weights"} if spectra else set()) | ({"images"} if n_img else set())
    np.testing.assert_array_equal(ch["SUM_WEIGHTS"], blk[L.CHAN["SUM_WEIGHTS"]:t * 8:8])
    if spectra:
        assert ch["energy_weights"].shape == (t, ne + 1)
        np.testing.assert_array_equal(ch["energy_weights"][:, 2], ch["SUM_WEIGHTS"])
    if n_img:
        assert ch["images"].shape == (t, n_img, n_img)
        np.testing.assert_allclose(ch["images"].sum(axis=(1, 2)) + ch["SUM_WEIGHTS_OUTSIDE"], ch["SUM_WEIGHTS"], rtol=1e-15)
    ch["names"] = list(R.COUPLINGS)
    paths = R.write_channel_csvs(str(tmp_path), "2018", ch, np.linspace(0.1, 0.6, ne), 14.0, 1.0, 2.0)
    assert [os.path.basename(p) for p in paths] == (["flux_by_channel_2018.csv"] + (["energies_by_channel_2018.csv"] if spectra else []) +
                                                    (["axion_image_2018_%s.csv" % n for n in R.COUPLINGS] if n_img else []))
    tab = R.read_flux_by_channel_csv(paths[0])
    assert list(tab) == ["channel", "name", "contributing rays", "flux", "flux error", "flux fraction"]
    assert tab["name"] == list(R.COUPLINGS)
    np.testing.assert_array_equal(tab["channel"], np.arange(t))
    np.testing.assert_array_equal(tab["contributing rays"], ch["N_CONTRIBUTING"])
    np.testing.assert_array_equal(tab["flux"], ch["SUM_WEIGHTS"])
    np.testing.assert_array_equal(tab["flux error"], np.sqrt(ch["SUM_WEIGHTS_SQ"]))
    assert tab["flux fraction"].sum() == pytest.approx(1.0, rel=1e-15)
    if spectra:
        eb = np.loadtxt(paths[1], delimiter=",", skiprows=1, ndmin=2, usecols=(0, 2, 3, 4))
        assert set(eb[:, 1].astype(int)) == {2}
        np.testing.assert_array_equal(eb[:, 3], ch["SUM_WEIGHTS"])
    if n_img:
        for k, p in enumerate(paths[-t:]):
            z = np.loadtxt(p, delimiter=",", skiprows=1, usecols=2)
            assert z.size == n_img * n_img and z.sum() == pytest.approx(ch["images"][k].sum(), rel=1e-15)


def _synthetic_rays(t=3, n=500, seed=11):
    """Per-ray contributions c[ray][t] = w f_t of rays shared by the channels, and the channels dict a trace would return."""
    rng = np.random.default_rng(seed)
    w = rng.random(n) * 1e-3
    f = rng.random((n, t))
    f /= f.sum(axis=1, keepdims=True)
    c = w[:, None] * f
    e_idx = rng.integers(0, 5, n)
    en = np.zeros((t, 6))
    for k in range(t):
        np.add.at(en[k], e_idx, c[:, k])
    ch = {"SUM_WEIGHTS": c.sum(axis=0), "SUM_WEIGHTS_SQ": (c * c).sum(axis=0), "N_CONTRIBUTING": np.full(t, float(n)),
          "SUM_WEIGHTS_OUTSIDE": np.zeros(t), "energy_weights": en, "images": rng.random((t, 4, 4)),
          "names": list(R.COUPLINGS), "couplings": list(R.COUPLINGS)}
    return c, ch


def test_coupling_signal_is_the_plain_sum_at_the_reference_and_quadratic_in_each_coupling():
    c, ch = _synthetic_rays()
    ref = R.coupling_signal(ch)
    assert np.all(ref["scale"] == 1.0)
    assert ref["flux"] == pytest.approx(ch["SUM_WEIGHTS"].sum(), rel=1e-15)
    np.testing.assert_allclose(ref["energy_weights"], ch["energy_weights"].sum(axis=0), rtol=1e-15)
    np.testing.assert_allclose(ref["image"], ch["images"].sum(axis=0), rtol=1e-15)
    same = R.coupling_signal(ch, **R.REFERENCE_COUPLINGS)
    assert same["flux"] == ref["flux"] and same["flux_error"] == ref["flux_error"]
    for k, name in enumerate(R.COUPLINGS):
        for factor in (0.5, 3.0):
            s = R.coupling_signal(ch, **{name: factor * R.REFERENCE_COUPLINGS[name]})
            want = ch["SUM_WEIGHTS"].sum() + (factor ** 2 - 1.0) * ch["SUM_WEIGHTS"][k]
            assert s["flux"] == pytest.approx(want, rel=1e-14), (name, factor)
            np.testing.assert_allclose(s["image"], ch["images"].sum(axis=0) + (factor ** 2 - 1.0) * ch["images"][k], rtol=1e-13)
            np.testing.assert_allclose(s["energy_weights"], ch["energy_weights"].sum(axis=0) + (factor ** 2 - 1.0) * ch["energy_weights"][k],
                                       rtol=1e-13, atol=1e-300)
    # another reference: the same signal when both move together
    s = R.coupling_signal(ch, g_ae=2e-13, ref={"g_ae": 2e-13})
    assert s["flux"] == ref["flux"]
    # channels that share a coupling (grouping "terms") scale together
    ch8 = dict(ch, couplings=["g_ae", "g_ae", "g_anuclei"])
    s = R.coupling_signal(ch8, g_ae=2e-13)
    assert s["flux"] == pytest.approx(4.0 * (ch["SUM_WEIGHTS"][0] + ch["SUM_WEIGHTS"][1]) + ch["SUM_WEIGHTS"][2], rel=1e-14)
    with pytest.raises(ValueError):
        R.coupling_signal(dict(ch, couplings=None))


def test_coupling_signal_error_is_a_bound_on_the_exact_error():
    c, ch = _synthetic_rays()
    for g in ({}, {"g_ae": 3e-13}, {"g_agamma": 0.1e-12, "g_anuclei": 7e-15}, {"g_ae": 0.0}):
        s = R.coupling_signal(ch, **g)
        exact = np.sqrt(((c * s["scale"][None, :]).sum(axis=1) ** 2).sum())   # the rays are shared: sqrt(sum_rays (sum_t s_t c_t)^2)
        assert s["flux_error"] >= exact * (1.0 - 1e-14), g


def test_group_emission_components():
    comp = np.arange(8 * 2 * 3, dtype=np.float64).reshape(8, 2, 3)
    rates, names, couplings = R.group_emission_components(comp, "terms")
    assert rates is not None and names == list(L.EM_TERMS) and couplings == [R.TERM_COUPLING[t] for t in L.EM_TERMS]
    np.testing.assert_array_equal(rates, comp)
    rates, names, couplings = R.group_emission_components(comp, "couplings")
    assert names == couplings == list(R.COUPLINGS) and rates.shape == (3, 2, 3)
    np.testing.assert_array_equal(rates.sum(axis=0), comp.sum(axis=0))
    with pytest.raises(ValueError):
        R.group_emission_components(comp, "shells")


def test_term_to_coupling_map_against_the_cpu_oracle():
    """Doubling exactly one coupling multiplies exactly that group's terms by 4 and leaves the others bit-equal - with every one of
    the eight terms positive in many of the compared cells, so that no entry of the map could move unnoticed."""
    from oracle import oracle as O
    assert set(R.TERM_COUPLING) == set(L.EM_TERMS) and set(R.TERM_COUPLING.values()) == set(R.COUPLINGS)
    zones = em.solar_zones()
    _, energies = tables.solar_grid()
    rs, es = 246, 1   # every energy: the 57Fe line is a few bins wide
    # term1 and the transverse plasmon conversion are proportional to the absorption coefficient, and the longitudinal resonance is a
    # few cells wide without it: a flat synthetic coefficient makes all three non-zero over the grid (the map does not depend on it)
    abs_coefs = np.full((len(zones), energies.size), 1.0)
    dbl_min = np.finfo(np.float64).tiny
    base_p = em.default_params()
    assert {c: getattr(base_p, c) for c in R.COUPLINGS} == R.REFERENCE_COUPLINGS
    _, base = O.emission_table(zones, energies, base_p, abs_coefs=abs_coefs, components=True, r_stride=rs, e_stride=es)
    base = base[:, ::rs, ::es]
    assert np.isfinite(base).all() and base.shape[1] >= 8 and base.shape[2] >= 8
    for coupling in R.COUPLINGS:
        p = em.default_params()
        setattr(p, coupling, 2.0 * getattr(p, coupling))
        _, comp = O.emission_table(zones, energies, p, abs_coefs=abs_coefs, components=True, r_stride=rs, e_stride=es)
        comp = comp[:, ::rs, ::es]
        for k, term in enumerate(L.EM_TERMS):
            # results below DBL_MIN - the far tails of the 57Fe line - are subnormal doubles, which carry fewer than 53 bits: they are
            # left out of the relative comparison; every other cell is held to rtol
            ok = ~(((comp[k] > 0.0) & (comp[k] < dbl_min)) | ((base[k] > 0.0) & (4.0 * base[k] < dbl_min)))
            assert (base[k][ok] > 0.0).sum() >= 50, (term, int((base[k][ok] > 0.0).sum()))     # the comparison is not empty
            if R.TERM_COUPLING[term] == coupling:
                np.testing.assert_allclose(comp[k][ok], 4.0 * base[k][ok], rtol=1e-12, atol=0, err_msg="%s / %s" % (term, coupling))
                assert np.all(comp[k][~ok] < 4.0 * dbl_min)
            else:
                np.testing.assert_array_equal(comp[k], base[k], err_msg="%s / %s" % (term, coupling))


def _parse(argv):
    ap = build_parser()
    args = ap.parse_args(argv)
    check_scan_args(ap, args)
    return args


def test_cli_accepts_both_groupings():
    assert _parse(["--emissionChannels", "terms"]).emissionChannels == "terms"
    assert _parse(["--emissionChannels", "couplings"]).emissionChannels == "couplings"
    assert _parse([]).emissionChannels is None
    with pytest.raises(SystemExit) as e:
        _parse(["--emissionChannels", "shells"])
    assert e.value.code == 2


@pytest.mark.parametrize("grouping", ["terms", "couplings"])
@pytest.mark.parametrize("extra", [["--massScanMin", "0", "--massScanMax", "0.02"],
                                   ["--angularScanMin", "0", "--angularScanMax", "0.1"],
                                   ["--xrayTest", "--energyScanMin", "1", "--energyScanMax", "8"],
                                   ["--xrayTest"]])
def test_cli_refuses_the_channels_beside_a_scan_or_the_test_source(grouping, extra, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(["--emissionChannels", grouping] + extra)
    assert e.value.code == 2
    assert "cannot be combined" in capsys.readouterr().err


def test_cli_refuses_the_channels_beside_shell_breakdown(capsys):
    with pytest.raises(SystemExit) as e:
        _parse(["--emissionChannels", "terms", "--shellBreakdown"])
    assert e.value.code == 2 and "cannot be combined" in capsys.readouterr().err


def test_cli_refuses_the_channels_beside_a_solar_model_csv_before_building_anything(tmp_path, capsys):
    """A config whose solar-model CSV exists: exit 2 from the arguments and the file system alone; without the file the run goes on."""
    (tmp_path / "config").mkdir()
    (tmp_path / "resources").mkdir()
    cfg = tmp_path / "config" / "config.toml"
    cfg.write_text('[Resources]\nresourcePath = "../resources"\nsolarModelFile = "solar_model.csv"\n')
    ap = build_parser()
    for argv in (["--config", str(cfg)], ["--configPath", str(tmp_path / "config")]):
        args = ap.parse_args(["--emissionChannels", "couplings"] + argv)
        check_channels_config(ap, args)                      # no such file yet: nothing to refuse
        check_channels_config(ap, ap.parse_args(argv))       # and nothing without the switch
    (tmp_path / "resources" / "solar_model.csv").write_text("Radius,Energy,emRate\n")
    check_channels_config(ap, ap.parse_args(["--config", str(cfg)]))
    for argv in (["--config", str(cfg)], ["--configPath", str(tmp_path / "config")]):
        with pytest.raises(SystemExit) as e:
            check_channels_config(ap, ap.parse_args(["--emissionChannels", "couplings"] + argv))
        err = capsys.readouterr().err
        assert e.value.code == 2 and "cannot be combined" in err and "solar_model.csv" in err
