"""Command line of the reference's `raytracer` binary (`proc main`, raytracer.nim:2817-2865) on top of the GPU path.

    python -m solaraxionraytracing_amd [--ignoreDetWindow] [--ignoreGasAbs] [--ignoreConvProb] [--ignoreReflection]
        [--xrayTest] [--detectorInstall] [--magnet] [--angularScanMin A --angularScanMax B --numAngularScanPoints N]
        [--fusedAngularScan] [--angularImages]
        [--noPlots] [--config FILE | --configPath DIR]  [--rays N] [--seed S] [--outpath DIR]
        [--massScanMin M0 --massScanMax M1 --numMassScanPoints K]     (not in the reference: see below)
        [--massScanBands N [--massScanBandMin keV --massScanBandMax keV]]  (with the mass scan: see below)
        [--energyScanMin E0 --energyScanMax E1 --numEnergyScanPoints K]  (not in the reference: see below)
        [--shellBreakdown]                                               (not in the reference: see below)
        [--emissionChannels {terms,couplings}]                           (not in the reference: see below)
        [--events PATH.npz [--eventColumns a,b,c]]                       (not in the reference: see below)
        [--originMap]                                                    (not in the reference: see below)
        [--apertureMap [--apertureBins N] [--apertureWindow x0,x1,y0,y1]]  (not in the reference: see below)

Same switches, same two modes (full run = calculateFluxFractions, :2755-2776; angular scan, :2778-2815).  What differs:
`--rays` replaces the compile-time constant NumberOfPointsSun (:251, default 1e6), plots are never made (the numbers
behind them are written as CSV), and without a config file the setup is that of config_default.toml
(BabyIAXO / InGridIAXO / vacuum / XMM, config_default.toml:19-22) with the synthetic input tables of tables.py.
A third mode the reference does not have (it has one constant mAxion, :255): --massScanMin / --massScanMax / --numMassScanPoints
run the fused axion-mass scan (every ray traced once, weighed for every mass; `stageSetup = "gas"` in the config, else the flux does
not depend on the mass) and write `axion_mass_scan.csv`.
With --massScanBands N (gas stage) the same trace also splits every mass's signal into N energy bands (1 .. 31; uniform in the index
of the energy table, over the whole table or over [--massScanBandMin, --massScanBandMax] keV, which must lie on cell edges) and
writes `axion_mass_scan_spectra.csv`: one row per mass and band - band edges, flux, its error sqrt(sum of w^2), the axions of the
band on the detector - and per mass one last row (band N, edges nan) for everything outside the bands, so that a mass's rows add up
to its flux in `axion_mass_scan.csv`.
A fourth: --energyScanMin / --energyScanMax / --numEnergyScanPoints (keV) run the fused energy scan of the X-ray test source
(`--xrayTest` or the config's [TestXraySource]; every ray traced once, weighed at every energy) and write `energy_scan.csv`: the
detection efficiency per energy and, for a parallel beam, the effective area (the quantity of the reference's
llnl_xray_telescope_cast_effective_area_parallel_light_DTU_thesis.csv).  It cannot be combined with the other scans.
--shellBreakdown (full-run mode only) also breaks the result down by mirror shell (Axion.shellNumber, :218; the data of
generateResultPlots' dfDet "Shell" column and energies_by_shell plot, :2351-2376) and writes `shell_breakdown_{year}.csv` and
`energies_by_shell_{year}.csv` beside the image CSV.
--emissionChannels terms|couplings (full-run mode only) also breaks the result down by the process that emitted the axion: the eight
terms of the solar emission table (readOpacityFile.nim:849) or their sums per coupling (g_ae, g_agamma, g_anuclei), from the one trace.
The run's emission table becomes the all-terms AGSS09 table made on the GPU (the only one whose components are known: it cannot be
combined with --xrayTest or a solar-model CSV, nor with --shellBreakdown: one breakdown per run).  Writes `flux_by_channel_{year}.csv`, `energies_by_channel_{year}.csv` and one
`axion_image_{year}_{name}.csv` per channel.
--events PATH.npz (full-run mode only) also writes the passed rays themselves, as columns in ray order (the `axionsPass` that
generateResultPlots plots from, :2253-2289): one array per name of --eventColumns (default pointdataX, pointdataY, pointdataR,
energiesAx, weights, shellNumber, ray_id; any field of the Axion record, `flags`, `kinds_packed`, `ray_id`) and the four counts
n_rays, n_passed, n_passed_till_window, n_hit_nickel.  The rays are those of the image: same seed, same ids.
--originMap (full-run mode only; not beside --xrayTest, --shellBreakdown or --emissionChannels: one breakdown per run) also keeps the
detected weight per cell (solar radius, energy) of the emission table the passed rays were drawn in, from the one trace, and writes
`origin_map_{year}.npz` (counts, weights, weights_sq [n_radii][n_energies], radii, energies, n_rays and the traced rates) and
`flux_by_solar_radius_{year}.csv`.  `python -m solaraxionraytracing_amd.reweight origin_map_{year}.npz --solarModel FILE.csv` then
gives the flux for another solar model on the same grid without a new trace (origin.py).
--apertureMap (full-run mode only; allowed with --xrayTest; not beside --shellBreakdown, --emissionChannels or --originMap: one
breakdown per run) also keeps the detected weight per cell of a grid over the telescope's entrance plane (pointEntranceXRT, the
record's pointdataXBefore / pointdataYBefore, :2091-2094), from the one trace: --apertureBins N (default 256) cells a side over
--apertureWindow x0,x1,y0,y1 in mm (default: the square of +-1.02 x the largest R1 of the setup's shells about the optical axis).
Writes `aperture_map_{year}.npz` (counts, weights, weights_sq [ny][nx], outside, x_edges, y_edges, n_rays, head) and
`aperture_image_{year}.csv` (x, y, N, flux, sigma) and prints the share of the flux that entered outside the window (aperture.py)."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from . import _lib, aperture, config as cfgmod, origin
from .raytracer import (RayTracer, energy_bands, angle_image_names, containment_radii, initFullSetup, performAngularScan, performAxionMassScan,
                        performEnergyScan, write_channel_csvs, write_image_csv, write_shell_csvs)

WINDOW_YEAR = {_lib.DK_INGRID2017: "2017", _lib.DK_INGRID2018: "2018", _lib.DK_INGRIDIAXO: "IAXO"}   # WindowYearKind, :1468-1484


EVENT_COLUMNS = ("pointdataX", "pointdataY", "pointdataR", "energiesAx", "weights", "shellNumber", "ray_id")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m solaraxionraytracing_amd", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    for name in ("ignoreDetWindow", "ignoreGasAbs", "ignoreConvProb", "ignoreReflection", "xrayTest", "detectorInstall",
                 "magnet", "noPlots"):
        ap.add_argument("--" + name, action="store_true")
    ap.add_argument("--angularScanMin", type=float, default=0.0)
    ap.add_argument("--angularScanMax", type=float, default=0.0)
    ap.add_argument("--numAngularScanPoints", type=int, default=50)
    ap.add_argument("--fusedAngularScan", action="store_true",
                    help="extension: the angular scan through the fused kernel (sart_trace_angular_scan: every ray sampled once and "
                         "turned through every angle, the same rays for all angles) instead of a re-trace on fresh rays per angle")
    ap.add_argument("--angularImages", action="store_true",
                    help="extension: the angular scan also writes every angle's focal-plane image, axion_image_{year}_angle_{a:.2f}.csv "
                         "(the reference's per-angle calculateFluxFractions without --noPlots), and prints its counters and means; "
                         "angles that share a name at two decimals get the fewest decimals that tell them apart (equal angles: "
                         "their index behind the name)")
    ap.add_argument("--massScanMin", type=float, default=0.0, help="eV (extension: fused axion-mass scan)")
    ap.add_argument("--massScanMax", type=float, default=0.0, help="eV")
    ap.add_argument("--numMassScanPoints", type=int, default=32)
    ap.add_argument("--massScanBands", type=int, default=0, metavar="N",
                    help="extension (mass scan, gas stage): also the signal per energy band and mass, axion_mass_scan_spectra.csv; "
                         "N bands (1 .. 31) over the whole energy table, or over [--massScanBandMin, --massScanBandMax]")
    ap.add_argument("--massScanBandMin", type=float, default=None, metavar="keV", help="lower edge of the bands (a cell edge of the energy table)")
    ap.add_argument("--massScanBandMax", type=float, default=None, metavar="keV", help="upper edge of the bands")
    ap.add_argument("--energyScanMin", type=float, default=0.0, help="keV (extension: fused energy scan of the X-ray test source)")
    ap.add_argument("--energyScanMax", type=float, default=0.0, help="keV")
    ap.add_argument("--numEnergyScanPoints", type=int, default=32)
    ap.add_argument("--shellBreakdown", action="store_true",
                    help="extension (full-run mode): the result per mirror shell, shell_breakdown_{year}.csv and energies_by_shell_{year}.csv")
    ap.add_argument("--emissionChannels", choices=("terms", "couplings"), default=None,
                    help="extension (full-run mode): the result per emission process (terms) or per coupling (couplings) from the one "
                         "trace; switches the emission table to the all-terms AGSS09 table made on the GPU")
    ap.add_argument("--originMap", action="store_true",
                    help="extension (full-run mode): the detected flux per (solar radius, energy) cell of the emission table, "
                         "origin_map_{year}.npz and flux_by_solar_radius_{year}.csv; reweightable to another solar model "
                         "(python -m solaraxionraytracing_amd.reweight)")
    ap.add_argument("--apertureMap", action="store_true",
                    help="extension (full-run mode): the detected flux per cell of a grid over the telescope's entrance plane, "
                         "aperture_map_{year}.npz and aperture_image_{year}.csv")
    ap.add_argument("--apertureBins", type=int, default=256, metavar="N", help="cells a side of --apertureMap (default: %(default)s)")
    ap.add_argument("--apertureWindow", default="", metavar="x0,x1,y0,y1",
                    help="window of --apertureMap in mm (default: +-1.02 x the largest R1 of the setup's shells)")
    ap.add_argument("--events", default="", metavar="PATH.npz",
                    help="extension (full-run mode): the passed rays as columns, in ray order, and the four counts, as a numpy .npz")
    ap.add_argument("--eventColumns", default=",".join(EVENT_COLUMNS), help="comma-separated columns of --events (default: %(default)s)")
    ap.add_argument("--config", default="", help="path of a config.toml")
    ap.add_argument("--configPath", default="", help="directory that holds config.toml")
    ap.add_argument("--rays", type=float, default=1e6, help="NumberOfPointsSun (raytracer.nim:251)")
    ap.add_argument("--seed", type=int, default=299792458)
    ap.add_argument("--outpath", default="out")
    ap.add_argument("--device", type=int, default=0)
    return ap


def energy_scan_requested(args) -> bool:
    return args.energyScanMin != 0.0 or args.energyScanMax != 0.0


def check_scan_args(ap: argparse.ArgumentParser, args) -> None:
    """The energy scan is a mode of its own: exits 2 (argparse's usage error) when it is combined with another scan or asks for
    no valid energies.  --shellBreakdown and --events belong to the full-run mode: exit 2 beside any scan."""
    if getattr(args, "events", "") and (energy_scan_requested(args) or args.massScanMax > args.massScanMin
                                        or args.angularScanMin != args.angularScanMax):
        ap.error("--events belongs to the full run: it cannot be combined with a mass, angular or energy scan")
    if getattr(args, "events", ""):
        unknown = [c for c in event_columns(args) if c not in _lib.COLUMNS]
        if unknown or not event_columns(args):
            ap.error("--eventColumns: unknown column(s) %s; known: %s" % (", ".join(unknown) or "(none given)", ", ".join(_lib.COLUMNS)))
    if getattr(args, "shellBreakdown", False) and (energy_scan_requested(args) or args.massScanMax > args.massScanMin
                                                   or args.angularScanMin != args.angularScanMax):
        ap.error("--shellBreakdown belongs to the full run: it cannot be combined with a mass, angular or energy scan")
    if getattr(args, "emissionChannels", None):
        if energy_scan_requested(args) or args.massScanMax > args.massScanMin or args.angularScanMin != args.angularScanMax:
            ap.error("--emissionChannels belongs to the full run: it cannot be combined with a mass, angular or energy scan")
        if args.xrayTest:
            ap.error("--emissionChannels needs the solar source: it cannot be combined with --xrayTest")
        if getattr(args, "shellBreakdown", False):
            ap.error("--emissionChannels cannot be combined with --shellBreakdown (one breakdown per run)")
    if getattr(args, "originMap", False):
        if energy_scan_requested(args) or args.massScanMax > args.massScanMin or args.angularScanMin != args.angularScanMax:
            ap.error("--originMap belongs to the full run: it cannot be combined with a mass, angular or energy scan")
        if args.xrayTest:
            ap.error("--originMap needs the solar source: it cannot be combined with --xrayTest")
        if getattr(args, "shellBreakdown", False) or getattr(args, "emissionChannels", None):
            ap.error("--originMap cannot be combined with --shellBreakdown or --emissionChannels (one breakdown per run)")
    if getattr(args, "apertureMap", False):
        if energy_scan_requested(args) or args.massScanMax > args.massScanMin or args.angularScanMin != args.angularScanMax:
            ap.error("--apertureMap belongs to the full run: it cannot be combined with a mass, angular or energy scan")
        if getattr(args, "shellBreakdown", False) or getattr(args, "emissionChannels", None) or getattr(args, "originMap", False):
            ap.error("--apertureMap cannot be combined with --shellBreakdown, --emissionChannels or --originMap (one breakdown per run)")
        if not 1 <= args.apertureBins <= min(_lib.APERTURE_MAX_SIDE, int(_lib.APERTURE_MAX_CELLS ** 0.5)):
            ap.error("--apertureMap: --apertureBins must lie in [1, %d]" % min(_lib.APERTURE_MAX_SIDE, int(_lib.APERTURE_MAX_CELLS ** 0.5)))
        if args.apertureWindow:
            try:
                x0, x1, y0, y1 = aperture_window(args)
            except ValueError:
                ap.error("--apertureMap: --apertureWindow takes four numbers x0,x1,y0,y1")
            if not (np.all(np.isfinite([x0, x1, y0, y1])) and x1 > x0 and y1 > y0):
                ap.error("--apertureMap: --apertureWindow needs finite x0 < x1 and y0 < y1")
    if getattr(args, "massScanBands", 0) or getattr(args, "massScanBandMin", None) is not None or getattr(args, "massScanBandMax", None) is not None:
        if not args.massScanMax > args.massScanMin:
            ap.error("--massScanBands belongs to the mass scan: it needs --massScanMin < --massScanMax")
        if energy_scan_requested(args) or args.angularScanMin != args.angularScanMax:
            ap.error("--massScanBands cannot be combined with an angular or energy scan")
        if not 1 <= args.massScanBands <= _lib.MSPEC_MAX_BANDS:
            ap.error("--massScanBands must lie in [1, %d]" % _lib.MSPEC_MAX_BANDS)
        if (args.massScanBandMin is None) != (args.massScanBandMax is None):
            ap.error("--massScanBands: give both --massScanBandMin and --massScanBandMax, or neither")
        if args.massScanBandMin is not None and not (np.isfinite([args.massScanBandMin, args.massScanBandMax]).all()
                                                     and args.massScanBandMin < args.massScanBandMax):
            ap.error("--massScanBands needs finite --massScanBandMin < --massScanBandMax (keV)")
    if not energy_scan_requested(args):
        return
    if args.massScanMax > args.massScanMin or args.angularScanMin != args.angularScanMax:
        ap.error("--energyScanMin / --energyScanMax cannot be combined with a mass scan or an angular scan")
    if not (0.0 < args.energyScanMin < args.energyScanMax) or args.numEnergyScanPoints < 1:
        ap.error("the energy scan needs 0 < --energyScanMin < --energyScanMax (keV) and --numEnergyScanPoints >= 1")


def config_path_of(args) -> str:
    return args.config or (os.path.join(args.configPath, "config.toml") if args.configPath else "")


def check_channels_config(ap: argparse.ArgumentParser, args) -> None:
    """--emissionChannels beside a config whose solar-model CSV exists: exit 2 before anything is built (a CSV has no components)."""
    path = config_path_of(args)
    if getattr(args, "emissionChannels", None) and path:
        csv = cfgmod.solar_model_csv_of(path)
        if csv:
            ap.error("--emissionChannels cannot be combined with a solar-model CSV (%s): its components are not known" % csv)


def aperture_window(args, full=None):
    """(x0, x1, y0, y1) of --apertureWindow; without it the square of +-1.02 x the largest R1 of ``full``'s shells."""
    if args.apertureWindow:
        x0, x1, y0, y1 = (float(v) for v in args.apertureWindow.split(","))
        return x0, x1, y0, y1
    half = 1.02 * max(full.setup.all_r1[:full.setup.n_shells])
    return -half, half, -half, half


def mass_scan_bands(ap: argparse.ArgumentParser, args, full):
    """((e0, width, n_bands), edges in keV) of --massScanBands: the requested window, or the whole energy table in N bands of the
    largest whole width that fits (the indices left over at the top land in the outside cell).  Exits 2 for a request the
    table's index grid cannot represent, and outside the gas stage."""
    if full.setup.stage != _lib.SK_GAS:
        ap.error("--massScanBands needs the gas stage (the vacuum conversion probability does not depend on the axion mass)")
    en = np.asarray(full.energies, dtype=np.float64)
    try:
        if args.massScanBandMin is not None:
            return energy_bands(en, args.massScanBandMin, args.massScanBandMax, args.massScanBands)
        step = (en[-1] - en[0]) / (en.size - 1)
        width = en.size // args.massScanBands
        if width < 1:
            raise ValueError("--massScanBands: the energy table has fewer points (%d) than bands" % en.size)
        lo = en[0] - 0.5 * step
        return energy_bands(en, lo, lo + step * width * args.massScanBands, args.massScanBands)
    except ValueError as e:
        ap.error(str(e))


def event_columns(args) -> list:
    return [c.strip() for c in args.eventColumns.split(",") if c.strip()]


def setup_from_args(args):
    flags = cfgmod.flags_from_cli(args.ignoreDetWindow, args.ignoreGasAbs, args.ignoreConvProb, args.ignoreReflection,
                                  args.xrayTest, args.detectorInstall, args.magnet)
    path = config_path_of(args)
    over = {"emission": "agss09"} if getattr(args, "emissionChannels", None) else {}
    if path:
        return cfgmod.init_full_setup_from_config(path, flags, **over), flags
    return initFullSetup(flags=flags, **over), flags


def write_result(path, img, s, spec, chip_max):
    """The numbers of generateResultPlots (:2252-2257, :2276-2278, :2459-2527) and the heat map's CSV (:885-921)."""
    print("Passed axions", int(s["N_PASSED"]))
    print("Passed axions until the Window", int(s["N_PASSED_TILL_WINDOW"]))
    print("Number of X-rays hitting nickel:", int(s["N_HIT_NICKEL"]))
    if s["N_PASSED"] > 0:   # means of the passed rays' detector coordinates (:2276-2278)
        print("mean x %.6f mean y %.6f mean r %.6f" % tuple(s[k] / s["N_PASSED"] for k in ("SUM_X", "SUM_Y", "SUM_R")))
    r1, r2, r1w, r2w = containment_radii(spec)
    print("rSigma1 %.4f rSigma2 %.4f rSigma1W %.4f rSigma2W %.4f" % (r1, r2, r1w, r2w))
    flux = write_image_csv(path, img, chip_max, r1w, r2w)
    print("The total flux", flux)
    print("wrote", path)


def main(argv=None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    check_scan_args(ap, args)
    check_channels_config(ap, args)
    full, flags = setup_from_args(args)
    if energy_scan_requested(args) and not full.setup.test_active:
        ap.error("the energy scan needs the X-ray test source: --xrayTest, or [TestXraySource] active in the config")
    if args.emissionChannels:
        if full.setup.test_active:
            ap.error("--emissionChannels needs the solar source: the config's X-ray test source is active")
        if full.meta.get("emission") != "E0-agss09-all-terms-gpu":
            ap.error("--emissionChannels cannot be combined with a solar-model CSV (%s): its components are not known"
                     % full.meta.get("emission"))
        print("--emissionChannels: the emission table of this run is the all-terms AGSS09 table made on the GPU")
    if args.originMap:
        if full.setup.test_active:
            ap.error("--originMap needs the solar source: the config's X-ray test source is active")
        if full.em_rates is None:
            ap.error("--originMap needs the emission table on the host (this setup makes it on the device: %s)" % full.meta.get("emission"))
    if args.massScanBands:
        bands, band_edges = mass_scan_bands(ap, args, full)
    n = int(args.rays)
    os.makedirs(args.outpath, exist_ok=True)
    print("Flags:", [name for name, bit in (("cfIgnoreDetWindow", _lib.CF_IGNORE_DET_WINDOW), ("cfIgnoreGasAbs", _lib.CF_IGNORE_GAS_ABS),
                                            ("cfIgnoreReflection", _lib.CF_IGNORE_REFLECTION), ("cfIgnoreConvProb", _lib.CF_IGNORE_CONV_PROB),
                                            ("cfXrayTest", _lib.CF_XRAY_TEST), ("cfReadMagnetConfig", _lib.CF_READ_MAGNET_CONFIG),
                                            ("cfReadDetInstallConfig", _lib.CF_READ_DET_INSTALL_CONFIG)) if flags & bit])
    with RayTracer(full, device=args.device) as rt:
        if energy_scan_requested(args):
            energies = np.linspace(args.energyScanMin, args.energyScanMax, args.numEnergyScanPoints)
            res = performEnergyScan(rt, energies, n, seed=args.seed, flags=flags)
            n_rays = res["shared"]["N_RAYS"]
            area = res["effective_area_cm2"] if res["effective_area_cm2"] is not None else np.full(energies.size, np.nan)
            out = os.path.join(args.outpath, "energy_scan.csv")
            with open(out, "w") as f:
                f.write("Energy [keV],efficiency,efficiency error,passed X-rays,effective area [cm^2]\n")
                for e, eff, sg, k, a in zip(energies, res["efficiency"], res["sigma"], res["n_passed"], area):
                    f.write("%r,%r,%r,%d,%r\n" % (float(e), float(eff), float(sg / n_rays), int(k), float(a)))
            print("energy scan: %d energies on %d rays, maximum efficiency %.6g at %.6g keV"
                  % (energies.size, n, float(np.max(res["efficiency"])), float(energies[int(np.argmax(res["efficiency"]))])))
            print("wrote", out)
        elif args.massScanMax > args.massScanMin:
            masses = np.linspace(args.massScanMin, args.massScanMax, args.numMassScanPoints)
            if args.massScanBands:
                res = performAxionMassScan(rt, masses, n, seed=args.seed, flags=flags, bands=bands)
                fluxes, errs, n_pass = res["flux"], res["sigma"], res["n_passed"]
                out = os.path.join(args.outpath, "axion_mass_scan_spectra.csv")
                lo_edges = np.append(band_edges[:-1], np.nan)      # the last row of a mass: everything outside the window
                hi_edges = np.append(band_edges[1:], np.nan)
                with open(out, "w") as f:
                    f.write("m_a [eV],band,E min [keV],E max [keV],flux,flux error,axions on detector\n")
                    for k, m in enumerate(masses):
                        for b in range(bands[2] + 1):
                            f.write("%r,%d,%r,%r,%r,%r,%d\n" % (float(m), b, float(lo_edges[b]), float(hi_edges[b]), float(res["band_flux"][k, b]),
                                                               float(res["band_sigma"][k, b]), int(res["band_counts"][b])))
                print("mass scan spectra: %d bands of %d energy indices from index %d (%.6g - %.6g keV), %d of %d axions on the detector "
                      "outside them" % (bands[2], bands[1], bands[0], band_edges[0], band_edges[-1], int(res["band_counts"][-1]),
                                        int(res["band_counts"].sum())))
                print("wrote", out)
            else:
                fluxes, errs, n_pass = performAxionMassScan(rt, masses, n, seed=args.seed, flags=flags, errors=True)
            out = os.path.join(args.outpath, "axion_mass_scan.csv")
            with open(out, "w") as f:
                f.write("m_a [eV],flux,flux error,passed axions,relative flux\n")
                for m, fl, e, k in zip(masses, fluxes, errs, n_pass):
                    f.write("%r,%r,%r,%d,%r\n" % (float(m), float(fl), float(e), int(k), float(fl / fluxes.max())))
            print("mass scan: %d masses on %d rays, maximum at m_a = %.6g eV" % (masses.size, n, masses[int(np.argmax(fluxes))]))
            print("wrote", out)
        elif args.angularScanMin == args.angularScanMax:
            # calculateFluxFractions + the numbers of generateResultPlots (:2252-2257, :2459-2527, :885-921)
            year = WINDOW_YEAR.get(full.setup.detector_kind, "IAXO")
            if args.shellBreakdown:
                img, s, spec, shells = rt.trace_shells(n, seed=args.seed, flags=flags)
            elif args.emissionChannels:
                rt.set_emission_channels(args.emissionChannels)
                img, s, spec, chans = rt.trace_channels(n, seed=args.seed, flags=flags)
            elif args.originMap:
                img, s, spec, omap = rt.trace_origin(n, seed=args.seed, flags=flags)
            elif args.apertureMap:
                rt.set_aperture_grid(args.apertureBins, args.apertureBins, *aperture_window(args, full))
                img, s, spec, amap = rt.trace_aperture(n, seed=args.seed, flags=flags)
            else:
                img, s, spec = rt.trace_spectra(n, seed=args.seed, flags=flags)
            write_result(os.path.join(args.outpath, "axion_image_%s.csv" % year), img, s, spec, full.setup.chip_x_max)
            if args.shellBreakdown:
                for path in write_shell_csvs(args.outpath, year, shells, full.energies, s["N_RAYS"]):
                    print("wrote", path)
            if args.emissionChannels:
                r1w, r2w = containment_radii(spec)[2:]
                for path in write_channel_csvs(args.outpath, year, chans, full.energies, full.setup.chip_x_max, r1w, r2w):
                    print("wrote", path)
            if args.originMap:
                path = os.path.join(args.outpath, "origin_map_%s.npz" % year)
                np.savez_compressed(path, counts=omap["counts"], weights=omap["weights"], weights_sq=omap["weights_sq"], radii=full.radii,
                                    energies=full.energies, n_rays=np.float64(s["N_RAYS"]), rates=full.em_rates)
                print("wrote", path)
                print("wrote", origin.write_radial_csv(os.path.join(args.outpath, "flux_by_solar_radius_%s.csv" % year), omap, full.radii))
            if args.apertureMap:
                print("wrote", aperture.save_map(os.path.join(args.outpath, "aperture_map_%s.npz" % year), amap, s["N_RAYS"]))
                print("wrote", aperture.write_csv(os.path.join(args.outpath, "aperture_image_%s.csv" % year), amap))
                print("--apertureMap: %d x %d cells over x [%.6g, %.6g] y [%.6g, %.6g] mm; outside the window: %d passed axions, share of "
                      "the flux %.6g" % (args.apertureBins, args.apertureBins, amap["x_edges"][0], amap["x_edges"][-1], amap["y_edges"][0],
                                         amap["y_edges"][-1], int(amap["outside"]["N"]),
                                         aperture.reweight(amap, np.ones_like(amap["weights"]))["uncovered"]))
            if args.events:
                cols, counts = rt.trace_columns(n, event_columns(args), seed=args.seed, flags=flags)
                np.savez(args.events, **cols, **counts)
                print("wrote", args.events, "(%d passed rays, columns %s)" % (counts["n_passed"], ", ".join(cols)))
        else:
            res = performAngularScan(rt, args.angularScanMin, args.angularScanMax, args.numAngularScanPoints, n, seed=args.seed, flags=flags,
                                     fused=args.fusedAngularScan, errors=args.fusedAngularScan, images=args.angularImages)
            angles, fluxes, rel = res[:3]
            errs = res[3] if args.fusedAngularScan else [float("nan")] * len(angles)
            if args.angularImages:   # performAngularScan :2787: calculateFluxFractions(suffix = "_angle_{angle:.2f}") per angle
                imgs, summ, spec = res[-1]
                year = WINDOW_YEAR.get(full.setup.detector_kind, "IAXO")
                for a, name, img, s, sp in zip(angles, angle_image_names(year, angles), imgs, summ, spec):
                    print("angle %r deg:" % float(a))
                    write_result(os.path.join(args.outpath, name), img, s, sp, full.setup.chip_x_max)
            out = os.path.join(args.outpath, "angular_scan_telescope_y.csv")   # the reference only saves the PDF of this curve
            with open(out, "w") as f:
                f.write("Angles [deg],Flux fraction,relative flux,flux error\n")
                for a, fl, r, e in zip(angles, fluxes, rel, errs):
                    f.write("%r,%r,%r,%r\n" % (float(a), float(fl), float(r), float(e)))
            print("wrote", out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
