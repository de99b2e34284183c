"""Host-side mirror of the reference's driver layer for the per-ray hot path, in the reference's
vocabulary (src/raytracer.nim): ``initFullSetup`` -> ``FullRaytraceSetup``; ``traceAxionWrapper``;
``calculateFluxFractions``; ``performAngularScan``.

This module is plumbing: it builds the inputs (through the C++ host library) and calls the C-ABI of
libsart.so.  All per-ray work happens in the HIP kernels; there is no CPU path here.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib, tables
from ._lib import (AXION_DTYPE, Setup, Summary, TraceParams)  # noqa: F401


def newFullSetup(experiment: int, detector: int, stage: int, telescope: int, flags: int = 0,
                 magnet_cfg=None, source_cfg=None, install_cfg=None) -> Setup:
    """newExperimentSetup + newDetectorSetup + module constants (raytracer.nim:1411-1423, :1464-1496, :248-272)."""
    host = _lib.load_host()
    s = Setup()
    _lib.check(host.sart_host_new_full_setup(
        experiment, detector, stage, telescope, flags,
        C.byref(magnet_cfg) if magnet_cfg is not None else None,
        C.byref(source_cfg) if source_cfg is not None else None,
        C.byref(install_cfg) if install_cfg is not None else None, C.byref(s)), host=True)
    return s


@dataclass
class FullRaytraceSetup:
    """FullRaytraceSetup, raytracer.nim:232-242 (centerVecs are derived from ``setup`` by the callee)."""
    setup: Setup
    energies: np.ndarray            # [nE] keV
    fluxRadiusCDF: np.ndarray       # [nR]
    diffFluxCDFs: np.ndarray        # [nR][nE]
    reflectivity: tables.ReflectivityGrid
    detector_tables: tables.DetectorTables
    flags: int = 0
    outpath: str = "out"
    meta: dict = field(default_factory=dict)
    # emission="agss09-device": the sampling tables are made on the GPU by the context that uploads this setup (emission
    # kernel -> CDFs -> guides, nothing crosses PCIe); fluxRadiusCDF / diffFluxCDFs stay None until fetch_solar_tables()
    device_emission: dict | None = None
    # the grid and the emission table the CDFs were made from (None where the table exists on the device only): what a solar-origin
    # map is reweighted against (origin.py)
    radii: np.ndarray | None = None
    em_rates: np.ndarray | None = None

    def fetch_solar_tables(self, tracer: "RayTracer"):
        """Host copies of the CDFs a context built on the device (for the CPU oracle, plots, files)."""
        self.fluxRadiusCDF, self.diffFluxCDFs = tracer.solar_tables()
        return self

    def require_solar_tables(self):
        """Consumers that need the CDFs on the host (the CPU oracle, tools/make_golden*.py) call this: with
        emission="agss09-device" they exist on the GPU only until fetch_solar_tables(tracer) has copied them."""
        if self.fluxRadiusCDF is None or self.diffFluxCDFs is None:
            raise RuntimeError("this FullRaytraceSetup keeps its sampling tables on the device (emission=%r): call "
                               "full.fetch_solar_tables(tracer) with a RayTracer built from it first" % self.meta.get("emission"))
        return self


def initFullSetup(experiment: int = _lib.ES_BABYIAXO, detector: int = _lib.DK_INGRIDIAXO,
                  stage: int = _lib.SK_VACUUM, telescope: int = _lib.TK_XMM, flags: int = 0, *,
                  emission: str | np.ndarray = "primakoff", n_radii: int = tables.N_RADII,
                  n_energies: int = tables.N_ENERGIES, reflectivity: str | tables.ReflectivityGrid = "henke",
                  refl_n_angles: int = 1000, refl_n_energies: int = 1000, solar_model_csv: str | None = None,
                  magnet_cfg=None, source_cfg=None, install_cfg=None, opcd_path: str | None = None,
                  opcd_optional: bool = False) -> FullRaytraceSetup:
    """initFullSetup, raytracer.nim:2637-2753.  Defaults = config/config_default.toml:19-22
    (BabyIAXO / InGridIAXO / vacuum / XMM).  ``emission`` / ``reflectivity`` choose the synthetic stand-ins of
    tables.py when the reference's own input files are not available."""
    setup = newFullSetup(experiment, detector, stage, telescope, flags, magnet_cfg, source_cfg, install_cfg)
    dev_em = None
    if solar_model_csv is not None:
        radii, energies, em = tables.read_solar_model_csv(solar_model_csv)
        meta_em = "csv:" + solar_model_csv
    elif isinstance(emission, str) and emission == "legacy":   # E2: the reference's own emission_rates_Hz.txt / energies.txt (397 x 233)
        radii, energies, em = tables.legacy_emission_table()
        meta_em = "E2-legacy-emission_rates_Hz"
    else:
        radii, energies = tables.solar_grid(n_radii, n_energies)
        if isinstance(emission, np.ndarray):
            em, meta_em = emission, "user"
        elif emission == "primakoff":
            em, meta_em = tables.primakoff_emission_table(n_radii, n_energies), "E1-primakoff-agss09"
        elif emission == "agss09":   # all analytic terms of readOpacityFile.nim on the AGSS09 model, made on the GPU (BASELINE configs[4])
            from . import emission as _emission
            em, meta_em = _emission.agss09_emission_table(n_radii, n_energies)[2], "E0-agss09-all-terms-gpu"
        elif emission == "agss09-device":   # the same table, but it never leaves the GPU: RayTracer builds CDFs + guides on the device
            from . import emission as _emission
            zones = _emission.solar_zones(n_radii)
            dev_em = {"zones": zones, "params": _emission.default_params()}
            em, meta_em = None, "E0-agss09-all-terms-gpu-device-cdfs"
            if opcd_path is not None:   # with the absorption coefficients of the OPCD files (readOpacityFile.nim:731-745, :790-823)
                from . import opacity as _opacity
                try:
                    dev_em["opcd"] = _opacity.OpcdSet(opcd_path, zones)
                    dev_em["n_z"] = _opacity.number_densities(n_radii=n_radii)
                    dev_em["opcd_optional"] = bool(opcd_optional)
                    meta_em = "E0-agss09-all-terms-opcd-gpu-device-cdfs"
                except (_lib.SartError, OSError, ValueError) as e:
                    # opcd_optional (a config.toml that merely HAS an OPCD directory): an incomplete or unreadable set of files
                    # must not take the whole setup down - the table is made without the OPCD absorption term and says so
                    if not opcd_optional:
                        raise
                    dev_em.pop("opcd", None)
                    dev_em["notes"] = ["OPCD files in %s could not be loaded (%s): emission table without the OPCD absorption term" % (opcd_path, e)]
        elif emission == "flat":
            em, meta_em = tables.flat_emission_table(n_radii, n_energies), "E3-flat"
        else:
            raise ValueError("unknown emission table %r" % (emission,))
    rcdf, ecdf = tables.build_cdfs(em, radii, energies) if em is not None else (None, None)
    if isinstance(reflectivity, tables.ReflectivityGrid):
        refl, meta_r = reflectivity, "user"
    else:
        multi = setup.reflectivity_kind == _lib.RK_MULTI_COATING
        if reflectivity == "henke":
            refl = (tables.llnl_reflectivity_grids if multi else tables.gold_reflectivity_grid)(refl_n_angles, refl_n_energies)
            meta_r = "L1-henke-x4" if multi else "G1-henke-gold"
        elif reflectivity == "gold":   # single gold table on every shell (BASELINE config 2)
            refl, meta_r = tables.gold_reflectivity_grid(refl_n_angles, refl_n_energies), "G1-henke-gold"
            if multi:
                setup.reflectivity_kind = _lib.RK_SINGLE_COATING
                setup.n_coatings = 1
                setup.coating_layers[0] = setup.n_shells
        elif reflectivity == "analytic":
            refl = tables.analytic_reflectivity_grid(4 if multi else 1, refl_n_angles, refl_n_energies)
            meta_r = "G2-analytic"
        else:
            raise ValueError("unknown reflectivity %r" % (reflectivity,))
    det = tables.detector_tables()
    meta = {"emission": meta_em, "reflectivity": meta_r}
    if dev_em is not None and dev_em.get("notes"):
        meta["notes"] = list(dev_em["notes"])
    return FullRaytraceSetup(setup, np.ascontiguousarray(energies), rcdf, ecdf, refl, det, flags, meta=meta, device_emission=dev_em,
                             radii=np.ascontiguousarray(radii), em_rates=None if em is None else np.ascontiguousarray(em, dtype=np.float64))


def columns_from_records(records: np.ndarray, columns, ray_ids=None) -> dict:
    """The columns of RayTracer.trace_columns out of an AXION_DTYPE array (the records of the passed rays, in ray order):
    {name: 1-D array}, dtypes as there.  ``flags`` = passed | passedTillWindow << 8 | hitNickel << 16 and ``kinds_packed`` =
    kinds | kindsWindow << 8, as the library packs words 0 and 16 of the record; ``ray_id`` is no part of a record and comes
    from ``ray_ids`` (the global ids of these records)."""
    records = np.asarray(records)
    assert records.dtype == AXION_DTYPE
    u8 = lambda name: records[name].astype(np.uint64)
    cols = {}
    for c in sorted(set(columns), key=_lib.COLUMNS.__getitem__):
        if c == "flags":
            cols[c] = u8("passed") | (u8("passedTillWindow") << np.uint64(8)) | (u8("hitNickel") << np.uint64(16))
        elif c == "kinds_packed":
            cols[c] = u8("kinds") | (u8("kindsWindow") << np.uint64(8))
        elif c == "ray_id":
            if ray_ids is None:
                raise ValueError("the ray_id column is not in the records: pass ray_ids")
            cols[c] = np.ascontiguousarray(ray_ids, dtype=np.uint64)
            assert cols[c].shape == records.shape
        else:
            cols[c] = np.ascontiguousarray(records[c])
    return cols


class RayTracer:
    """One libsart context on one GPU holding the captures of ``traceAxionWrapper``
    (raytracer.nim:2223-2232)."""

    def __init__(self, full: FullRaytraceSetup, device: int = 0):
        self.lib = _lib.load_sart()
        self.full = full
        self.device = int(device)
        h = C.c_void_p()
        _lib.check(self.lib.sart_create(device, C.byref(h)))
        self.handle = h
        try:
            self._upload(full)
        except Exception:
            self.close()
            raise

    def _upload(self, full: FullRaytraceSetup):
        lib, h = self.lib, self.handle
        _lib.check(lib.sart_set_setup(h, C.byref(full.setup)))
        if full.device_emission is not None:
            # BASELINE configs[4]'s front end without a host round trip: emission kernel -> CDFs -> guide tables on the device
            de = full.device_emission
            done = False
            if de.get("opcd") is not None:
                try:
                    _lib.check(lib.sart_emission_to_solar_tables_opcd(h, de["zones"], len(de["zones"]), _lib.as_dp(de["n_z"]),
                                                                      _lib.as_dp(full.energies), full.energies.size, de["opcd"].tables,
                                                                      C.byref(de["params"])))
                    done = True
                except _lib.SartError as e:
                    # e.g. a (radius, energy) cell outside a table's abscissae (sart_opacity.hip): fatal unless the OPCD term
                    # was only an opportunistic upgrade (config.py), in which case the table is made without it - and says so
                    if not de.get("opcd_optional"):
                        raise
                    full.meta.setdefault("notes", []).append("OPCD absorption coefficients failed on the device (%s): emission table "
                                                             "without the OPCD absorption term" % e)
                    full.meta["emission"] = "E0-agss09-all-terms-gpu-device-cdfs"
            if not done:
                _lib.check(lib.sart_emission_to_solar_tables(h, de["zones"], len(de["zones"]), _lib.as_dp(full.energies),
                                                             full.energies.size, None, C.byref(de["params"])))
        else:
            n_r, n_e = full.diffFluxCDFs.shape
            _lib.check(lib.sart_set_solar_tables(h, _lib.as_dp(full.fluxRadiusCDF), _lib.as_dp(full.diffFluxCDFs),
                                                 _lib.as_dp(full.energies), n_r, n_e))
        r = full.reflectivity
        n_c, n_a, n_er = r.data.shape
        _lib.check(lib.sart_set_reflectivity(h, n_c, n_a, n_er, r.angle_min, r.angle_max, r.energy_min, r.energy_max,
                                             _lib.as_dp(r.data)))
        d = full.detector_tables
        _lib.check(lib.sart_set_detector_tables(h, _lib.as_dp(d.x_kev), _lib.as_dp(d.strongback), d.x_kev.size,
                                                _lib.as_dp(d.x_kev), _lib.as_dp(d.window), d.x_kev.size,
                                                _lib.as_dp(d.gas_x_kev), _lib.as_dp(d.gas_absorption), d.gas_x_kev.size))

    # -- lifecycle ----------------------------------------------------------------------------
    def close(self):
        if getattr(self, "handle", None):
            self.lib.sart_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- parameters ---------------------------------------------------------------------------
    def trace_params(self, n_rays: int, seed: int = 299792458, ray_id_offset: int = 0, flags: int | None = None,
                     image_n: int = 256, accumulate: bool = False) -> TraceParams:
        s = self.full.setup
        p = TraceParams()
        p.n_rays, p.seed, p.ray_id_offset = int(n_rays), int(seed), int(ray_id_offset)
        p.flags = self.full.flags if flags is None else flags
        p.image_nx = p.image_ny = image_n
        p.accumulate = 1 if accumulate else 0
        p.image_x_min, p.image_x_max = 0.0, s.chip_x_max      # beginX/endX (raytracer.nim:2622-2625)
        p.image_y_min, p.image_y_max = 0.0, s.chip_y_max
        return p

    def set_telescope_angles(self, turned_x_deg: float = float("nan"), turned_y_deg: float = float("nan")):
        _lib.check(self.lib.sart_set_telescope_angles(self.handle, turned_x_deg, turned_y_deg))

    def set_axion_mass(self, m_axion_ev: float):
        _lib.check(self.lib.sart_set_axion_mass(self.handle, m_axion_ev))

    def set_accumulation_mode(self, mode: int | str = _lib.ACCUM_F64, headroom_bits: int = 0):
        """SART_ACCUM_F64 (default: f64 atomics, as prepareHeatmap adds on the CPU) or SART_ACCUM_FIXED64 ("fixed64":
        integer accumulation, results bitwise independent of GPU count, replica placement and launch splitting;
        include/sart.h "accumulation mode").  The blocking calls keep returning doubles; trace_histogram_device then fills
        raw int64 accumulators (reduce them as int64, convert with finalize_accumulator_device)."""
        if isinstance(mode, str):
            mode = {"f64": _lib.ACCUM_F64, "fixed64": _lib.ACCUM_FIXED64}[mode]
        _lib.check(self.lib.sart_set_accumulation_mode(self.handle, int(mode), int(headroom_bits)))

    def accumulation_mode(self) -> int:
        m = C.c_int()
        _lib.check(self.lib.sart_get_accumulation_mode(self.handle, C.byref(m)))
        return m.value

    def fixed_quanta(self) -> dict:
        """The quanta the raw FIXED64 accumulators of this context count in (frozen by the first launch)."""
        q = _lib.FixedQuanta()
        _lib.check(self.lib.sart_get_fixed_quanta(self.handle, C.byref(q)))
        return {"weight": q.weight, "weight_sq": q.weight_sq, "position": q.position, "reflect": q.reflect}

    def finalize_accumulator_device(self, params: TraceParams, acc_fixed_ptr: int, out_f64_ptr: int | None = None):
        """Raw FIXED64 accumulator (device) -> f64 accumulator layout (device; in place by default).  Asynchronous."""
        _lib.check(self.lib.sart_finalize_accumulator_device(self.handle, C.byref(params), C.c_void_p(acc_fixed_ptr),
                                                             C.c_void_p(out_f64_ptr if out_f64_ptr is not None else acc_fixed_ptr)))

    def rollover_accumulator_device(self, params: TraceParams, acc_fixed_ptr: int, hi_limbs_ptr: int):
        """Long FIXED64 accumulations: moves the bits of every slot above 2^40 into the slot's limb in ``hi_limbs`` (device int64
        array of the accumulator's length, zeroed with it).  Asynchronous."""
        _lib.check(self.lib.sart_rollover_accumulator_device(self.handle, C.byref(params), C.c_void_p(acc_fixed_ptr), C.c_void_p(hi_limbs_ptr)))

    def finalize_accumulator_limbs_device(self, params: TraceParams, acc_fixed_ptr: int, hi_limbs_ptr: int | None, out_f64_ptr: int | None = None):
        """finalize_accumulator_device for an accumulator with roll-over limbs."""
        _lib.check(self.lib.sart_finalize_accumulator_limbs_device(self.handle, C.byref(params), C.c_void_p(acc_fixed_ptr),
                                                                   C.c_void_p(hi_limbs_ptr) if hi_limbs_ptr else None,
                                                                   C.c_void_p(out_f64_ptr if out_f64_ptr is not None else acc_fixed_ptr)))

    def set_solar_tables_device(self, em_rates_device_ptr: int, radii: np.ndarray, energies: np.ndarray):
        """sart_set_solar_tables_device: CDFs + guide tables built on the device from a device-resident emission table
        [n_radii][n_energies] (``torch_tensor.data_ptr()``)."""
        radii = np.ascontiguousarray(radii, dtype=np.float64)
        energies = np.ascontiguousarray(energies, dtype=np.float64)
        _lib.check(self.lib.sart_set_solar_tables_device(self.handle, C.c_void_p(em_rates_device_ptr), _lib.as_dp(radii),
                                                         _lib.as_dp(energies), radii.size, energies.size))
        self.full.energies = energies
        self._n_radii_set = radii.size
        self._chan_labels = None   # the library dropped the channels with the old tables

    def solar_tables(self, guides: bool = False):
        """Host copies of (fluxRadiusCDF, diffFluxCDFs) as the context holds them; with ``guides`` also the library's
        guide tables (radius guide [_lib.RADIUS_GUIDE_ENTRIES], energy guide [n_radii][_lib.ENERGY_GUIDE_ENTRIES], u16)."""
        n_e = self.full.energies.size
        n_r = self._n_radii()
        rcdf, ecdf = np.empty(n_r), np.empty((n_r, n_e))
        rg = np.empty(_lib.RADIUS_GUIDE_ENTRIES, dtype=np.uint16) if guides else None
        eg = np.empty((n_r, _lib.ENERGY_GUIDE_ENTRIES), dtype=np.uint16) if guides else None
        _lib.check(self.lib.sart_get_solar_tables(self.handle, _lib.as_dp(rcdf), _lib.as_dp(ecdf),
                                                  rg.ctypes.data_as(C.c_void_p) if guides else None,
                                                  eg.ctypes.data_as(C.c_void_p) if guides else None))
        return (rcdf, ecdf, rg, eg) if guides else (rcdf, ecdf)

    def radial_table(self):
        """The radial verdict table of the next histogram launch: (breakpoints [n] f64, verdict words [n] u32, cells [lut_n] u8),
        or None if this setup runs the compares (include/sart.h: sart_get_radial_table)."""
        b, w, cells = np.empty(128), np.empty(128, dtype=np.uint32), np.empty(1024, dtype=np.uint8)
        n_cells = C.c_int32(0)
        n = self.lib.sart_get_radial_table(self.handle, _lib.as_dp(b), w.ctypes.data_as(C.c_void_p), cells.ctypes.data_as(C.c_void_p),
                                           C.byref(n_cells))
        if n < 0:
            _lib.check(n)
        return (b[:n].copy(), w[:n].copy(), cells[:n_cells.value].copy()) if n > 0 else None

    def _n_radii(self) -> int:
        if getattr(self, "_n_radii_set", None):
            return self._n_radii_set
        if self.full.device_emission is not None:
            return len(self.full.device_emission["zones"])
        if self.full.diffFluxCDFs is not None:
            return self.full.diffFluxCDFs.shape[0]
        raise RuntimeError("number of radii unknown")

    def set_stream(self, hip_stream: int | None):
        _lib.check(self.lib.sart_set_stream(self.handle, C.c_void_p(hip_stream) if hip_stream else None))

    def synchronize(self):
        _lib.check(self.lib.sart_synchronize(self.handle))

    # -- the hot path -------------------------------------------------------------------------
    def traceAxionWrapper(self, bufLen: int, seed: int = 299792458, ray_id_offset: int = 0,
                          flags: int | None = None) -> np.ndarray:
        """traceAxionWrapper (raytracer.nim:2223-2244): ``bufLen`` Axion records (numpy structured array with
        the reference's field names)."""
        buf = np.zeros(bufLen, dtype=AXION_DTYPE)
        p = self.trace_params(bufLen, seed, ray_id_offset, flags)
        _lib.check(self.lib.sart_trace_records(self.handle, C.byref(p), buf.ctypes.data_as(C.c_void_p)))
        return buf

    def traceAxionWrapperPassed(self, bufLen: int, seed: int = 299792458, ray_id_offset: int = 0, flags: int | None = None,
                                capacity: int | None = None, out: np.ndarray | None = None):
        """The rays of traceAxionWrapper(bufLen, ...) whose ``passed`` is set, in ray order, and the counts generateResultPlots
        echoes (raytracer.nim:2252-2257): (records, {"n_rays", "n_passed", "n_passed_till_window", "n_hit_nickel"}).  Only the
        passed records cross PCIe (sart_trace_records_passed).  ``capacity`` = room of the buffer in records (default bufLen:
        always enough); ``out`` = a buffer of the caller's.  len(records) = min(n_passed, capacity)."""
        if out is None:
            out = np.empty(bufLen if capacity is None else capacity, dtype=AXION_DTYPE)
        assert out.dtype == AXION_DTYPE and out.flags.c_contiguous
        capacity = len(out) if capacity is None else min(int(capacity), len(out))
        p = self.trace_params(bufLen, seed, ray_id_offset, flags)
        cnt = _lib.RecordCounts()
        _lib.check(self.lib.sart_trace_records_passed(self.handle, C.byref(p), out.ctypes.data_as(C.c_void_p), capacity, C.byref(cnt)))
        counts = {k: int(getattr(cnt, k)) for k, _ in _lib.RecordCounts._fields_}
        return out[:min(counts["n_passed"], capacity)], counts

    def trace_records_passed_device(self, params: TraceParams, out_ptr: int, capacity: int, counts_ptr: int):
        """sart_trace_records_passed_device: device pointers (records, four uint64 counts); enqueues on the stream."""
        _lib.check(self.lib.sart_trace_records_passed_device(self.handle, C.byref(params), C.c_void_p(out_ptr), int(capacity), C.c_void_p(counts_ptr)))

    # -- the passed rays as selected columns (include/sart.h: sart_trace_columns_passed) --------
    DEFAULT_COLUMNS = ("pointdataX", "pointdataY", "pointdataR", "energiesAx", "weights", "shellNumber")

    def trace_columns(self, n: int, columns=DEFAULT_COLUMNS, seed: int = 299792458, ray_id_offset: int = 0, flags: int | None = None,
                      capacity: int | None = None, out: np.ndarray | None = None):
        """The passed rays of traceAxionWrapper(n, ...) as the named columns (_lib.COLUMNS), in ray order: ({name: 1-D array},
        counts as traceAxionWrapperPassed returns them).  Each array holds min(n_passed, capacity) entries and is a view of one
        [K][capacity] buffer of 8-byte slots (``out``: a C-contiguous uint64 array of the caller's with at least that many
        elements; ``capacity`` defaults to n, which is always enough): float64, except shellNumber (int64) and flags /
        kinds_packed / ray_id (uint64).  Only these words cross PCIe."""
        names = sorted(set(columns), key=_lib.COLUMNS.__getitem__)
        mask = _lib.column_mask(names)
        n_cols = bin(mask).count("1")      # (two names of one word, as "flags" and nothing else today, would share a column)
        capacity = int(n if capacity is None else capacity)
        if out is None:
            out = np.empty(n_cols * capacity, dtype=np.uint64)
        assert out.dtype == np.uint64 and out.flags.c_contiguous and out.size >= n_cols * capacity
        p = self.trace_params(n, seed, ray_id_offset, flags)
        cnt = _lib.RecordCounts()
        _lib.check(self.lib.sart_trace_columns_passed(self.handle, C.byref(p), mask, out.ctypes.data_as(C.c_void_p) if out.size else None,
                                                      capacity, C.byref(cnt)))
        counts = {k: int(getattr(cnt, k)) for k, _ in _lib.RecordCounts._fields_}
        m = min(counts["n_passed"], capacity)
        flat = out.reshape(-1)
        slot = {bit: j for j, bit in enumerate(sorted({_lib.COLUMNS[c] for c in names}))}
        return {c: flat[slot[_lib.COLUMNS[c]] * capacity:][:m].view(_lib.column_dtype(c)) for c in names}, counts

    def trace_columns_device(self, params: TraceParams, columns, capacity: int, out=None, counts=None):
        """sart_trace_columns_passed_device on torch tensors of the context's device: ({name: 1-D tensor of ``capacity`` slots},
        counts tensor of four int64).  The tensors are views of ``out``, one [K, capacity] int64 buffer (made here unless
        given): float64 for the doubles, int64 for shellNumber, flags, kinds_packed and ray_id.  Only enqueues on the context's
        stream: slots at and behind counts[1] keep what ``out`` held.  ``params.accumulate`` appends behind counts[1]."""
        import torch
        names = sorted(set(columns), key=_lib.COLUMNS.__getitem__)
        mask = _lib.column_mask(names)
        bits = sorted({_lib.COLUMNS[c] for c in names})
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.empty((len(bits), int(capacity)), dtype=torch.int64, device=dev)
        if counts is None:
            counts = torch.zeros(4, dtype=torch.int64, device=dev)
        assert out.dtype == torch.int64 and out.is_contiguous() and out.numel() >= len(bits) * int(capacity) and out.device == dev
        assert counts.dtype == torch.int64 and counts.is_contiguous() and counts.numel() >= 4 and counts.device == dev
        _lib.check(self.lib.sart_trace_columns_passed_device(self.handle, C.byref(params), mask, C.c_void_p(out.data_ptr()) if out.numel() else None,
                                                             int(capacity), C.c_void_p(counts.data_ptr())))
        rows = out.reshape(-1)[:len(bits) * int(capacity)].view(len(bits), int(capacity))
        cols = {}
        for c in names:
            row = rows[bits.index(_lib.COLUMNS[c])]
            cols[c] = row.view(torch.float64) if _lib.column_dtype(c) == np.float64 else row
        return cols, counts

    def trace_records_uniforms(self, uniforms: np.ndarray, flags: int | None = None) -> np.ndarray:
        """Test entry (sart_internal_trace_records_uniforms, not part of include/sart.h): the records of the rays whose six
        uniforms are the rows of ``uniforms`` [n][6] (draw order of SURVEY App. B) instead of draws from the Philox stream."""
        u = np.ascontiguousarray(uniforms, dtype=np.float64)
        assert u.ndim == 2 and u.shape[1] == 6
        buf = np.zeros(u.shape[0], dtype=AXION_DTYPE)
        p = self.trace_params(u.shape[0], flags=flags)
        fn = self.lib.sart_internal_trace_records_uniforms
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(TraceParams), C.c_void_p, C.c_void_p]
        _lib.check(fn(self.handle, C.byref(p), u.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p)))
        return buf

    def trace_histogram(self, n_rays: int, seed: int = 299792458, ray_id_offset: int = 0, flags: int | None = None,
                        image_n: int = 256, accumulate: bool = False):
        """Fused trace + prepareHeatmap(256,256,norm=1) + flux sum + counters.  Returns (image[ny][nx], summary
        dict keyed like include/sart.h SART_ACC_*)."""
        p = self.trace_params(n_rays, seed, ray_id_offset, flags, image_n, accumulate)
        img = np.empty((image_n, image_n))
        summ = Summary()
        _lib.check(self.lib.sart_trace_histogram(self.handle, C.byref(p), _lib.as_dp(img), C.byref(summ)))
        return img, {k: summ.v[i] for k, i in _lib.ACC.items()}

    def trace_image(self, n_rays: int, nx: int, ny: int, x_range=None, y_range=None, seed: int = 299792458,
                    ray_id_offset: int = 0, flags: int | None = None):
        """prepareHeatmap with any binning / window (raytracer.nim:818-842): e.g. the 3000 x 3000 maps of
        generateResultPlots (:2626, :2630).  Returns (image[ny][nx], summary)."""
        p = self.trace_params(n_rays, seed, ray_id_offset, flags, 1, False)
        p.image_nx, p.image_ny = int(nx), int(ny)
        if x_range is not None:
            p.image_x_min, p.image_x_max = float(x_range[0]), float(x_range[1])
        if y_range is not None:
            p.image_y_min, p.image_y_max = float(y_range[0]), float(y_range[1])
        img = np.empty((ny, nx))
        summ = Summary()
        _lib.check(self.lib.sart_trace_histogram(self.handle, C.byref(p), _lib.as_dp(img), C.byref(summ)))
        return img, {k: summ.v[i] for k, i in _lib.ACC.items()}

    def y_slice_histogram(self, n_rays: int, half_width: float = 0.05, bin_width: float = 0.001, **kw):
        """`y_{year}.pdf` of generateResultPlots (raytracer.nim:2551-2559): weighted histogram (bin 0.001 mm) of the
        y-positions of the rays with |x - ChipCenterX| < 0.05 mm — one image column.  Returns (bin edges, flux per bin)."""
        s = self.full.setup
        cx = 0.5 * s.chip_x_max
        ny = int(round(s.chip_y_max / bin_width))
        img, _ = self.trace_image(n_rays, 1, ny, x_range=(cx - half_width, cx + half_width), y_range=(0.0, s.chip_y_max), **kw)
        return np.linspace(0.0, s.chip_y_max, ny + 1), img[:, 0].copy()

    def trace_spectra(self, n_rays: int, seed: int = 299792458, ray_id_offset: int = 0, flags: int | None = None,
                      image_n: int = 256, n_radial_bins: int = 10_000, radial_max: float = 10.0, accumulate: bool = False):
        """trace_histogram plus the post-processing histograms of generateResultPlots accumulated on the device:
        radial distribution (bin 0.001 mm by default, raytracer.nim:2386) and per-energy-index spectra.  Returns
        (image, summary, spectra dict)."""
        p = self.trace_params(n_rays, seed, ray_id_offset, flags, image_n, accumulate)
        p.spectra, p.n_radial_bins, p.radial_max = 1, n_radial_bins, radial_max
        n_e1 = self.full.energies.size + 1
        img = np.empty((image_n, image_n))
        summ = Summary()
        spec = np.empty(2 * n_radial_bins + 3 * n_e1)
        _lib.check(self.lib.sart_trace_histogram_spectra(self.handle, C.byref(p), _lib.as_dp(img), C.byref(summ), _lib.as_dp(spec)))
        return img, {k: summ.v[i] for k, i in _lib.ACC.items()}, split_spectra(spec, n_radial_bins, n_e1, radial_max)

    def trace_histogram_device(self, params: TraceParams, accumulator_ptr: int):
        """Asynchronous form: adds into a device accumulator (e.g. ``torch_tensor.data_ptr()``)."""
        _lib.check(self.lib.sart_trace_histogram_device(self.handle, C.byref(params), C.c_void_p(accumulator_ptr)))

    # -- per-shell breakdown (include/sart.h "per-shell breakdown of the histogram trace") -----
    def shell_block_len(self, spectra: bool = True) -> int:
        """sart_shell_block_len for this context's setup and energy table."""
        return int(self.lib.sart_shell_block_len(self.full.setup.n_shells, self.full.energies.size, 1 if spectra else 0))

    def shells_params(self, n_rays: int, seed: int = 299792458, ray_id_offset: int = 0, flags: int | None = None, image_n: int = 256,
                      spectra: bool = True, n_radial_bins: int = 10_000, radial_max: float = 10.0, accumulate: bool = False) -> TraceParams:
        """The TraceParams of trace_shells (for the _device form)."""
        p = self.trace_params(n_rays, seed, ray_id_offset, flags, image_n, accumulate)
        if spectra:
            p.spectra, p.n_radial_bins, p.radial_max = 1, n_radial_bins, radial_max
        return p

    def trace_shells(self, n_rays: int, seed: int = 299792458, ray_id_offset: int = 0, flags: int | None = None, image_n: int = 256,
                     spectra: bool = True, n_radial_bins: int = 10_000, radial_max: float = 10.0):
        """trace_histogram (trace_spectra with ``spectra``) plus the per-shell breakdown (sart_trace_histogram_shells).  Returns
        (image, summary, spectra dict or None, shells dict of per-shell arrays keyed like _lib.SHELL, with ``spectra`` also
        ``energy_counts`` / ``energy_weights`` [n_shells][n_energies + 1], and ``coating`` / ``R1``)."""
        p = self.shells_params(n_rays, seed, ray_id_offset, flags, image_n, spectra, n_radial_bins, radial_max)
        n_e1 = self.full.energies.size + 1
        img = np.empty((image_n, image_n))
        summ = Summary()
        spec = np.empty(2 * n_radial_bins + 3 * n_e1) if spectra else None
        block = np.empty(self.shell_block_len(spectra))
        _lib.check(self.lib.sart_trace_histogram_shells(self.handle, C.byref(p), _lib.as_dp(img) if image_n else None, C.byref(summ),
                                                        _lib.as_dp(spec) if spectra else None, _lib.as_dp(block)))
        shells = split_shells(block, self.full.setup.n_shells, self.full.energies.size, spectra)
        shells["coating"] = shell_coatings(self.full.setup)
        shells["R1"] = np.array(self.full.setup.all_r1[:self.full.setup.n_shells])
        return (img, {k: summ.v[i] for k, i in _lib.ACC.items()},
                split_spectra(spec, n_radial_bins, n_e1, radial_max) if spectra else None, shells)

    def trace_shells_device(self, params: TraceParams, accumulator_ptr: int, shells_ptr: int):
        """Asynchronous form: adds into a device accumulator and a device block of shell_block_len(params.spectra) slots (raw int64 in
        fixed64 mode)."""
        _lib.check(self.lib.sart_trace_histogram_shells_device(self.handle, C.byref(params), C.c_void_p(accumulator_ptr),
                                                               C.c_void_p(shells_ptr)))

    def finalize_shells_device(self, params: TraceParams, raw_ptr: int, out_ptr: int | None = None):
        """Raw FIXED64 shell block (device) -> doubles (device; in place by default).  Asynchronous; what the conversion finds
        wrong is raised by the next ``synchronize()``."""
        _lib.check(self.lib.sart_finalize_shells_device(self.handle, C.byref(params), C.c_void_p(raw_ptr),
                                                        C.c_void_p(out_ptr if out_ptr is not None else raw_ptr)))

    # -- emission-channel breakdown (include/sart.h "emission-channel breakdown of the histogram trace") ----
    def set_source_channels(self, rates, total, names=None, couplings=None):
        """sart_set_source_channels: ``rates`` [T][n_radii][n_energies] (host array, the layout of emission_table's components) and
        ``total`` [n_radii][n_energies], the table the context's CDFs were made from.  The library keeps rates / total per cell.
        ``names`` / ``couplings``: one label and one coupling name (COUPLINGS) per channel, carried into trace_channels' result."""
        rates = np.ascontiguousarray(rates, dtype=np.float64)
        total = np.ascontiguousarray(total, dtype=np.float64)
        if rates.ndim != 3 or total.ndim != 2 or rates.shape[1:] != total.shape:
            raise ValueError("rates must be [T][n_radii][n_energies] and total [n_radii][n_energies]")
        _lib.check(self.lib.sart_set_source_channels(self.handle, _lib.as_dp(rates), _lib.as_dp(total), rates.shape[0], total.shape[0],
                                                     total.shape[1]))
        self._channel_labels(rates.shape[0], names, couplings)

    def set_source_channels_device(self, rates_ptr: int, total_ptr: int, n_channels: int, n_radii: int, n_energies: int, names=None,
                                   couplings=None):
        """sart_set_source_channels_device: the same from DEVICE memory (``torch_tensor.data_ptr()``), identical bits."""
        _lib.check(self.lib.sart_set_source_channels_device(self.handle, C.c_void_p(rates_ptr), C.c_void_p(total_ptr), int(n_channels),
                                                            int(n_radii), int(n_energies)))
        self._channel_labels(int(n_channels), names, couplings)

    def _channel_labels(self, t, names, couplings):
        """The labels of the channels just set (kept with their count: labels of another set of channels are never handed out)."""
        names = list(names) if names is not None else ["channel%d" % k for k in range(t)]
        couplings = list(couplings) if couplings is not None else None
        if len(names) != t or (couplings is not None and len(couplings) != t):
            raise ValueError("names / couplings must have one entry per channel (%d)" % t)
        self._chan_labels = (t, names, couplings)

    def _labels_of(self, t):
        """(names, couplings) of the context's t channels: the labels given when they were set, else channel0 .. and None."""
        kept = getattr(self, "_chan_labels", None)
        if kept is not None and kept[0] == t:
            return list(kept[1]), (list(kept[2]) if kept[2] is not None else None)
        return ["channel%d" % k for k in range(t)], None

    def clear_source_channels(self):
        _lib.check(self.lib.sart_clear_source_channels(self.handle))
        self._chan_labels = None

    def n_source_channels(self) -> int:
        t = C.c_int32()
        _lib.check(self.lib.sart_get_source_channels(self.handle, None, C.byref(t)))
        return t.value

    def source_channels(self) -> np.ndarray:
        """The fractions the context holds, [T][n_radii][n_energies] (0 where the total is 0)."""
        t = self.n_source_channels()
        out = np.empty((t, self._n_radii(), self.full.energies.size))
        _lib.check(self.lib.sart_get_source_channels(self.handle, _lib.as_dp(out), None))
        return out

    def set_emission_channels(self, grouping: str = "couplings"):
        """Channels of a setup whose emission table this library made (emission="agss09" / "agss09-device"): the eight terms of
        include/sart_emission.h (``grouping="terms"``) or their sums per coupling (``"couplings"``: g_ae, g_agamma, g_anuclei, by
        TERM_COUPLING).  The components come from emission.emission_table(..., components=True) and are summed per group in numpy."""
        from . import emission as _emission
        de = self.full.device_emission
        if de is not None:
            if de.get("opcd") is not None:
                raise ValueError("set_emission_channels: setups with OPCD absorption coefficients are not supported")
            zones, params = de["zones"], de["params"]
        elif self.full.meta.get("emission") == "E0-agss09-all-terms-gpu":
            zones, params = _emission.solar_zones(self._n_radii()), _emission.default_params()
        else:
            raise ValueError("set_emission_channels needs a setup made with emission=\"agss09\" or \"agss09-device\" (this one: %r)"
                             % self.full.meta.get("emission"))
        total, comp = _emission.emission_table(zones, self.full.energies, params=params, components=True, device=self.device)
        rates, names, couplings = group_emission_components(comp, grouping)
        self.set_source_channels(rates, total, names, couplings)
        return names

    def channel_block_len(self, spectra: bool = True, image_n: int = 256) -> int:
        """sart_channel_block_len for this context's channels and energy table."""
        return int(self.lib.sart_channel_block_len(self.n_source_channels(), self.full.energies.size, 1 if spectra else 0, image_n, image_n))

    channels_params = shells_params

    def trace_channels(self, n_rays: int, seed: int = 299792458, ray_id_offset: int = 0, flags: int | None = None, image_n: int = 256,
                       spectra: bool = True, n_radial_bins: int = 10_000, radial_max: float = 10.0):
        """trace_histogram (trace_spectra with ``spectra``) plus the emission-channel breakdown (sart_trace_histogram_channels).
        Returns (image, summary, spectra dict or None, channels dict of per-channel arrays keyed like _lib.CHAN, with ``spectra``
        also ``energy_weights`` [T][n_energies + 1], with an image ``images`` [T][ny][nx], and ``names`` / ``couplings``)."""
        p = self.channels_params(n_rays, seed, ray_id_offset, flags, image_n, spectra, n_radial_bins, radial_max)
        t, n_e = self.n_source_channels(), self.full.energies.size
        img = np.empty((image_n, image_n))
        summ = Summary()
        spec = np.empty(2 * n_radial_bins + 3 * (n_e + 1)) if spectra else None
        block = np.empty(_lib.channel_block_len(t, n_e, spectra, image_n, image_n))
        _lib.check(self.lib.sart_trace_histogram_channels(self.handle, C.byref(p), _lib.as_dp(img) if image_n else None, C.byref(summ),
                                                          _lib.as_dp(spec) if spectra else None, _lib.as_dp(block)))
        ch = split_channels(block, t, n_e, spectra, image_n, image_n)
        ch["names"], ch["couplings"] = self._labels_of(t)
        return (img, {k: summ.v[i] for k, i in _lib.ACC.items()},
                split_spectra(spec, n_radial_bins, n_e + 1, radial_max) if spectra else None, ch)

    def trace_channels_device(self, params: TraceParams, accumulator_ptr: int, channels_ptr: int):
        """Asynchronous form: adds into a device accumulator and a device block of channel_block_len(...) slots (raw int64 in fixed64
        mode).  With ``params.accumulate`` the library adds to what the buffers hold: whatever filled them (a ``torch.zeros`` on
        torch's stream, say) must have finished, or be ordered on the context's stream (``set_stream``), before this call."""
        _lib.check(self.lib.sart_trace_histogram_channels_device(self.handle, C.byref(params), C.c_void_p(accumulator_ptr),
                                                                 C.c_void_p(channels_ptr)))

    def finalize_channels_device(self, params: TraceParams, raw_ptr: int, out_ptr: int | None = None):
        """Raw FIXED64 channel block (device) -> doubles (device; in place by default).  Asynchronous; what the conversion finds wrong
        is raised by the next ``synchronize()``."""
        _lib.check(self.lib.sart_finalize_channels_device(self.handle, C.byref(params), C.c_void_p(raw_ptr),
                                                          C.c_void_p(out_ptr if out_ptr is not None else raw_ptr)))

    # -- solar-origin map (include/sart.h "solar-origin map of the histogram trace") -----------
    def origin_block_len(self) -> int:
        """sart_origin_block_len for this context's solar tables."""
        return int(self.lib.sart_origin_block_len(self._n_radii(), self.full.energies.size))

    origin_params = shells_params

    def trace_origin(self, n_rays: int, seed: int = 299792458, ray_id_offset: int = 0, flags: int | None = None, image_n: int = 256,
                     spectra: bool = True, n_radial_bins: int = 10_000, radial_max: float = 10.0):
        """trace_histogram (trace_spectra with ``spectra``) plus the solar-origin map (sart_trace_histogram_origin): the detected
        weight per cell (radius index, energy index) of the emission table the passed rays were drawn in.  Returns (image, summary,
        spectra dict or None, origin dict: ``head`` and the maps ``counts``, ``weights``, ``weights_sq`` [n_radii][n_energies]); see
        solaraxionraytracing_amd.origin for what the maps answer."""
        p = self.origin_params(n_rays, seed, ray_id_offset, flags, image_n, spectra, n_radial_bins, radial_max)
        n_r, n_e = self._n_radii(), self.full.energies.size
        img = np.empty((image_n, image_n))
        summ = Summary()
        spec = np.empty(2 * n_radial_bins + 3 * (n_e + 1)) if spectra else None
        block = np.empty(_lib.origin_block_len(n_r, n_e))
        _lib.check(self.lib.sart_trace_histogram_origin(self.handle, C.byref(p), _lib.as_dp(img) if image_n else None, C.byref(summ),
                                                        _lib.as_dp(spec) if spectra else None, _lib.as_dp(block)))
        return (img, {k: summ.v[i] for k, i in _lib.ACC.items()},
                split_spectra(spec, n_radial_bins, n_e + 1, radial_max) if spectra else None, split_origin(block, n_r, n_e))

    def trace_origin_device(self, params: TraceParams, accumulator_ptr: int, origin_ptr: int):
        """Asynchronous form: adds into a device accumulator and a device block of origin_block_len() slots (raw int64 in fixed64
        mode); ``params.accumulate`` as in trace_channels_device."""
        _lib.check(self.lib.sart_trace_histogram_origin_device(self.handle, C.byref(params), C.c_void_p(accumulator_ptr),
                                                               C.c_void_p(origin_ptr)))

    def finalize_origin_device(self, params: TraceParams, raw_ptr: int, out_ptr: int | None = None):
        """Raw FIXED64 origin block (device) -> doubles (device; in place by default).  Asynchronous; what the conversion finds wrong
        is raised by the next ``synchronize()``."""
        _lib.check(self.lib.sart_finalize_origin_device(self.handle, C.byref(params), C.c_void_p(raw_ptr),
                                                        C.c_void_p(out_ptr if out_ptr is not None else raw_ptr)))

    # -- aperture map (include/sart.h "aperture map of the histogram trace") --------------------
    def set_aperture_grid(self, nx: int, ny: int, x_min: float, x_max: float, y_min: float, y_max: float):
        """The grid of the aperture map (sart_set_aperture_grid): nx x ny cells over [x_min, x_max) x [y_min, y_max) of the entrance
        plane, mm in the telescope frame (the frame of pointdataXBefore / pointdataYBefore).  Context state, as the source channels."""
        g = _lib.ApertureGrid(int(nx), int(ny), float(x_min), float(x_max), float(y_min), float(y_max))
        _lib.check(self.lib.sart_set_aperture_grid(self.handle, C.byref(g)))

    def aperture_grid(self) -> dict:
        """The context's grid (sart_get_aperture_grid) as a dict nx, ny, x_min, x_max, y_min, y_max."""
        g = _lib.ApertureGrid()
        _lib.check(self.lib.sart_get_aperture_grid(self.handle, C.byref(g)))
        return {k: getattr(g, k) for k, _ in _lib.ApertureGrid._fields_}

    def aperture_block_len(self) -> int:
        """sart_aperture_block_len for this context's grid."""
        g = self.aperture_grid()
        return int(self.lib.sart_aperture_block_len(g["nx"], g["ny"]))

    aperture_params = shells_params

    def trace_aperture(self, n_rays: int, seed: int = 299792458, ray_id_offset: int = 0, flags: int | None = None, image_n: int = 256,
                       spectra: bool = True, n_radial_bins: int = 10_000, radial_max: float = 10.0):
        """trace_histogram (trace_spectra with ``spectra``) plus the aperture map (sart_trace_histogram_aperture): the detected weight
        per cell of the context's grid over the entrance plane (set_aperture_grid).  Returns (image, summary, spectra dict or None,
        aperture dict: ``head``, the maps ``counts``, ``weights``, ``weights_sq`` [ny][nx], ``outside`` and the grid's ``x_edges`` /
        ``y_edges``); see solaraxionraytracing_amd.aperture for what the maps answer."""
        p = self.aperture_params(n_rays, seed, ray_id_offset, flags, image_n, spectra, n_radial_bins, radial_max)
        g = self.aperture_grid()
        n_e = self.full.energies.size
        img = np.empty((image_n, image_n))
        summ = Summary()
        spec = np.empty(2 * n_radial_bins + 3 * (n_e + 1)) if spectra else None
        block = np.empty(_lib.aperture_block_len(g["nx"], g["ny"]))
        _lib.check(self.lib.sart_trace_histogram_aperture(self.handle, C.byref(p), _lib.as_dp(img) if image_n else None, C.byref(summ),
                                                          _lib.as_dp(spec) if spectra else None, _lib.as_dp(block)))
        amap = split_aperture(block, g["nx"], g["ny"])
        amap["x_edges"] = np.linspace(g["x_min"], g["x_max"], g["nx"] + 1)
        amap["y_edges"] = np.linspace(g["y_min"], g["y_max"], g["ny"] + 1)
        return (img, {k: summ.v[i] for k, i in _lib.ACC.items()},
                split_spectra(spec, n_radial_bins, n_e + 1, radial_max) if spectra else None, amap)

    def trace_aperture_device(self, params: TraceParams, accumulator_ptr: int, aperture_ptr: int):
        """Asynchronous form: adds into a device accumulator and a device block of aperture_block_len() slots (raw int64 in fixed64
        mode); ``params.accumulate`` as in trace_origin_device."""
        _lib.check(self.lib.sart_trace_histogram_aperture_device(self.handle, C.byref(params), C.c_void_p(accumulator_ptr),
                                                                 C.c_void_p(aperture_ptr)))

    def finalize_aperture_device(self, params: TraceParams, raw_ptr: int, out_ptr: int | None = None):
        """Raw FIXED64 aperture block (device) -> doubles (device; in place by default).  Asynchronous; what the conversion finds wrong
        is raised by the next ``synchronize()``."""
        _lib.check(self.lib.sart_finalize_aperture_device(self.handle, C.byref(params), C.c_void_p(raw_ptr),
                                                          C.c_void_p(out_ptr if out_ptr is not None else raw_ptr)))

    # -- fused axion-mass scan (gas stage; include/sart.h "fused axion-mass scan") -------------
    def trace_mass_scan(self, masses_ev, n_rays: int, seed: int = 299792458, ray_id_offset: int = 0, flags: int | None = None):
        """Every ray of [ray_id_offset, ray_id_offset + n_rays) traced ONCE and weighed for every axion mass.  Returns
        (per-mass dict of arrays SUM_WEIGHTS / SUM_WEIGHTS_SQ / N_PASSED, dict of the mass-independent counters)."""
        masses = np.ascontiguousarray(masses_ev, dtype=np.float64)
        p = self.trace_params(n_rays, seed, ray_id_offset, flags)
        out = np.empty(mass_scan_len(masses.size))
        _lib.check(self.lib.sart_trace_mass_scan(self.handle, C.byref(p), _lib.as_dp(masses), masses.size, _lib.as_dp(out)))
        return split_mass_scan(out, masses.size)

    def trace_mass_scan_device(self, params: TraceParams, masses_ev, scan_acc_ptr: int):
        """Asynchronous form: adds into a device scan accumulator of mass_scan_len(n) 8-byte slots (raw int64 in fixed64 mode)."""
        masses = np.ascontiguousarray(masses_ev, dtype=np.float64)
        _lib.check(self.lib.sart_trace_mass_scan_device(self.handle, C.byref(params), _lib.as_dp(masses), masses.size,
                                                        C.c_void_p(scan_acc_ptr)))

    def finalize_mass_scan_device(self, params: TraceParams, masses_ev, raw_ptr: int, out_ptr: int | None = None):
        """Raw FIXED64 scan accumulator (device) -> doubles (device; in place by default).  Asynchronous; what the conversion
        finds wrong (unresolved weights, wrapped slots) is raised by the next ``synchronize()``."""
        masses = np.ascontiguousarray(masses_ev, dtype=np.float64)
        _lib.check(self.lib.sart_finalize_mass_scan_device(self.handle, C.byref(params), _lib.as_dp(masses), masses.size,
                                                           C.c_void_p(raw_ptr), C.c_void_p(out_ptr if out_ptr is not None else raw_ptr)))

    # -- fused axion-mass scan with energy bands (include/sart.h "fused axion-mass scan with energy bands") ----
    def trace_mass_scan_spectra(self, masses_ev, bands, n_rays: int, seed: int = 299792458, ray_id_offset: int = 0,
                                flags: int | None = None):
        """trace_mass_scan with every mass's sums split by energy band.  ``bands`` = (e0, width, n_bands) in energy-index space
        (energy_bands() makes them from keV).  Returns (per-mass dict, shared-counter dict, spectra dict: ``SUM_WEIGHTS`` and
        ``SUM_WEIGHTS_SQ`` [n_masses][n_bands + 1] - the last cell is everything outside the window - and ``N_ON_DETECTOR``
        [n_bands + 1])."""
        masses = np.ascontiguousarray(masses_ev, dtype=np.float64)
        b = _lib.EnergyBands(*[int(v) for v in bands])
        p = self.trace_params(n_rays, seed, ray_id_offset, flags)
        out = np.empty(mass_scan_len(masses.size))
        spec = np.empty(_lib.mass_scan_spectra_len(masses.size, max(b.n_bands, 0)))
        _lib.check(self.lib.sart_trace_mass_scan_spectra(self.handle, C.byref(p), _lib.as_dp(masses), masses.size, C.byref(b),
                                                         _lib.as_dp(out), _lib.as_dp(spec)))
        return split_mass_scan(out, masses.size) + (split_mass_scan_spectra(spec, masses.size, b.n_bands),)

    def trace_mass_scan_spectra_device(self, params: TraceParams, masses_ev, bands, scan_acc_ptr: int, spectra_ptr: int):
        """Asynchronous form: adds into a device scan accumulator of mass_scan_len(n) slots and a device spectra buffer of
        mass_scan_spectra_len(n, n_bands) slots (raw int64 in fixed64 mode)."""
        masses = np.ascontiguousarray(masses_ev, dtype=np.float64)
        b = _lib.EnergyBands(*[int(v) for v in bands])
        _lib.check(self.lib.sart_trace_mass_scan_spectra_device(self.handle, C.byref(params), _lib.as_dp(masses), masses.size, C.byref(b),
                                                                C.c_void_p(scan_acc_ptr), C.c_void_p(spectra_ptr)))

    def finalize_mass_scan_spectra_device(self, params: TraceParams, masses_ev, bands, scan_raw_ptr: int, spectra_raw_ptr: int,
                                          out_ptr: int):
        """Raw FIXED64 scan rows and spectra (device) -> doubles in ``out_ptr`` (device; mass_scan_len(n) doubles, then
        mass_scan_spectra_len(n, n_bands); not in place).  Asynchronous; what the conversion finds wrong (a wrapped slot, cells that
        do not add up to their row, unresolved weights) is raised by the next ``synchronize()``."""
        masses = np.ascontiguousarray(masses_ev, dtype=np.float64)
        b = _lib.EnergyBands(*[int(v) for v in bands])
        _lib.check(self.lib.sart_finalize_mass_scan_spectra_device(self.handle, C.byref(params), _lib.as_dp(masses), masses.size, C.byref(b),
                                                                   C.c_void_p(scan_raw_ptr), C.c_void_p(spectra_raw_ptr), C.c_void_p(out_ptr)))

    # -- fused energy scan (X-ray test source; include/sart.h "fused energy scan") --------------
    def trace_energy_scan(self, energies_kev, n_rays: int, seed: int = 299792458, ray_id_offset: int = 0, flags: int | None = None):
        """Every ray of [ray_id_offset, ray_id_offset + n_rays) traced ONCE and weighed at every X-ray energy (keV) of the test
        source.  Returns (per-energy dict of arrays SUM_WEIGHTS / SUM_WEIGHTS_SQ / N_PASSED / N_PASSED_TILL_WINDOW, dict of the
        energy-independent counters)."""
        energies = np.ascontiguousarray(energies_kev, dtype=np.float64)
        p = self.trace_params(n_rays, seed, ray_id_offset, flags)
        out = np.empty(_lib.energy_scan_len(energies.size))
        _lib.check(self.lib.sart_trace_energy_scan(self.handle, C.byref(p), _lib.as_dp(energies), energies.size, _lib.as_dp(out)))
        return _lib.split_energy_scan(out, energies.size)

    def trace_energy_scan_device(self, params: TraceParams, energies_kev, scan_acc_ptr: int):
        """Asynchronous form: adds into a device scan accumulator of energy_scan_len(n) 8-byte slots (raw int64 in fixed64 mode)."""
        energies = np.ascontiguousarray(energies_kev, dtype=np.float64)
        _lib.check(self.lib.sart_trace_energy_scan_device(self.handle, C.byref(params), _lib.as_dp(energies), energies.size,
                                                          C.c_void_p(scan_acc_ptr)))

    def finalize_energy_scan_device(self, params: TraceParams, energies_kev, raw_ptr: int, out_ptr: int | None = None):
        """Raw FIXED64 energy-scan accumulator (device) -> doubles (device; in place by default).  Asynchronous; what the
        conversion finds wrong is raised by the next ``synchronize()``."""
        energies = np.ascontiguousarray(energies_kev, dtype=np.float64)
        _lib.check(self.lib.sart_finalize_energy_scan_device(self.handle, C.byref(params), _lib.as_dp(energies), energies.size,
                                                             C.c_void_p(raw_ptr), C.c_void_p(out_ptr if out_ptr is not None else raw_ptr)))

    # -- fused angular scan (include/sart.h "fused angular scan") -------------------------------
    def trace_angular_scan(self, turned_y_deg, n_rays: int, seed: int = 299792458, ray_id_offset: int = 0, flags: int | None = None):
        """Every ray of [ray_id_offset, ray_id_offset + n_rays) sampled and taken through bore and pipes ONCE and turned through
        every telescope angle.  Returns (per-angle dict of arrays SUM_WEIGHTS / SUM_WEIGHTS_SQ / N_PASSED / N_SHELL_SELECTED /
        N_HIT_NICKEL / N_PASSED_TILL_WINDOW, dict of the angle-independent counters)."""
        angles = np.ascontiguousarray(turned_y_deg, dtype=np.float64)
        p = self.trace_params(n_rays, seed, ray_id_offset, flags)
        out = np.empty(angular_scan_len(angles.size))
        _lib.check(self.lib.sart_trace_angular_scan(self.handle, C.byref(p), _lib.as_dp(angles), angles.size, _lib.as_dp(out)))
        return split_angular_scan(out, angles.size)

    def trace_angular_scan_device(self, params: TraceParams, turned_y_deg, scan_acc_ptr: int):
        """Asynchronous form: adds into a device scan accumulator of angular_scan_len(n) 8-byte slots (raw int64 in fixed64 mode)."""
        angles = np.ascontiguousarray(turned_y_deg, dtype=np.float64)
        _lib.check(self.lib.sart_trace_angular_scan_device(self.handle, C.byref(params), _lib.as_dp(angles), angles.size,
                                                           C.c_void_p(scan_acc_ptr)))

    def finalize_angular_scan_device(self, params: TraceParams, n_angles: int, raw_ptr: int, out_ptr: int | None = None):
        """Raw FIXED64 scan accumulator (device) -> doubles (device; in place by default).  Asynchronous."""
        _lib.check(self.lib.sart_finalize_angular_scan_device(self.handle, C.byref(params), int(n_angles), C.c_void_p(raw_ptr),
                                                              C.c_void_p(out_ptr if out_ptr is not None else raw_ptr)))

    def trace_angular_scan_images(self, turned_y_deg, n_rays: int, seed: int = 299792458, ray_id_offset: int = 0,
                                  flags: int | None = None, image_n: int = 256, spectra: bool = False, n_radial_bins: int = 10_000,
                                  radial_max: float = 10.0):
        """The fused angular scan with a complete accumulator per angle (sart_trace_angular_scan_images): per angle what
        trace_histogram / trace_spectra return after set_telescope_angles(turned_y_deg=a) on the same rays.  Returns (images
        [K, ny, nx], list of K summary dicts keyed like SART_ACC_*, list of K split_spectra dicts or None, the scan rows as
        trace_angular_scan returns them)."""
        angles = np.ascontiguousarray(turned_y_deg, dtype=np.float64)
        p = self.angular_scan_images_params(n_rays, seed, ray_id_offset, flags, image_n, spectra, n_radial_bins, radial_max)
        n_e1 = self.full.energies.size + 1
        blen = image_n * image_n + _lib.SART_ACC_COUNT + (2 * n_radial_bins + 3 * n_e1 if spectra else 0)
        rows = np.empty(angular_scan_len(angles.size))
        blocks = np.empty((angles.size, blen))
        _lib.check(self.lib.sart_trace_angular_scan_images(self.handle, C.byref(p), _lib.as_dp(angles), angles.size, _lib.as_dp(rows),
                                                           _lib.as_dp(blocks)))
        return split_image_blocks(blocks, image_n, n_radial_bins if spectra else 0, n_e1, radial_max) + (split_angular_scan(rows, angles.size),)

    def angular_scan_images_params(self, n_rays: int, seed: int = 299792458, ray_id_offset: int = 0, flags: int | None = None,
                                   image_n: int = 256, spectra: bool = False, n_radial_bins: int = 10_000, radial_max: float = 10.0,
                                   accumulate: bool = False) -> TraceParams:
        """The TraceParams of trace_angular_scan_images (for the _device form)."""
        p = self.trace_params(n_rays, seed, ray_id_offset, flags, image_n, accumulate)
        if spectra:
            p.spectra, p.n_radial_bins, p.radial_max = 1, n_radial_bins, radial_max
        return p

    def trace_angular_scan_images_device(self, params: TraceParams, turned_y_deg, scan_acc_ptr: int, blocks_ptr: int):
        """Asynchronous form: adds into a device scan accumulator of angular_scan_len(K) slots and K device accumulator blocks
        (raw int64 in fixed64 mode; finalize block by block with finalize_accumulator_device)."""
        angles = np.ascontiguousarray(turned_y_deg, dtype=np.float64)
        _lib.check(self.lib.sart_trace_angular_scan_images_device(self.handle, C.byref(params), _lib.as_dp(angles), angles.size,
                                                                  C.c_void_p(scan_acc_ptr), C.c_void_p(blocks_ptr)))

    def trace_flux(self, n_rays: int, seed: int = 299792458, ray_id_offset: int = 0, flags: int | None = None):
        """Flux-only launch (image_nx = image_ny = 0, include/sart.h): the summary of trace_histogram without an image."""
        p = self.trace_params(n_rays, seed, ray_id_offset, flags, 0, False)
        summ = Summary()
        _lib.check(self.lib.sart_trace_histogram(self.handle, C.byref(p), None, C.byref(summ)))
        return {k: summ.v[i] for k, i in _lib.ACC.items()}

    # -- measurement --------------------------------------------------------------------------
    def enable_kernel_timing(self, enable: bool = True):
        _lib.check(self.lib.sart_enable_kernel_timing(self.handle, 1 if enable else 0))

    def kernel_timing(self):
        ms, n = C.c_double(), C.c_int64()
        _lib.check(self.lib.sart_get_kernel_timing(self.handle, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def device_info(self):
        ncu, ws = C.c_int32(), C.c_int32()
        name = C.create_string_buffer(256)
        _lib.check(self.lib.sart_device_info(self.handle, C.byref(ncu), C.byref(ws), name, 256))
        return {"n_cu": ncu.value, "wave_size": ws.value, "name": name.value.decode()}


def split_spectra(spec: np.ndarray, n_radial_bins: int, n_e1: int, radial_max: float) -> dict:
    """Names the pieces of the spectra block of the accumulator (include/sart.h: sart_accumulator_len_spectra)."""
    o = 0
    out = {}
    for name, n in (("radial_counts", n_radial_bins), ("radial_weights", n_radial_bins), ("energy_counts", n_e1),
                    ("energy_weights", n_e1), ("energy_reflect", n_e1)):
        out[name] = spec[o:o + n].copy()
        o += n
    out["radial_max"] = radial_max
    return out


shell_block_len = _lib.shell_block_len
split_shells = _lib.split_shells


def shell_coatings(setup: Setup) -> np.ndarray:
    """Coating index of every shell as the library assigns it: layers.lowerBound(shell) over coating_layers for a multi-coating
    telescope (raytracer.nim:1573, the first boundary >= the shell index), coating 0 otherwise."""
    n = setup.n_shells
    if setup.reflectivity_kind != _lib.RK_MULTI_COATING:
        return np.zeros(n, dtype=np.int64)
    layers = np.array(setup.coating_layers[:setup.n_coatings])
    return np.searchsorted(layers, np.arange(n), side="left").astype(np.int64)


def write_shell_csvs(outpath: str, year: str, shells: dict, energies: np.ndarray, n_rays: float):
    """`shell_breakdown_{year}.csv` (per shell: coating, R1, the counters, flux, its Monte-Carlo error and its fraction of the
    total flux) and, with energy arrays in ``shells``, `energies_by_shell_{year}.csv` (the data of the reference's energies_by_shell
    plot, raytracer.nim:2361-2376: rays and flux per shell and energy bin; the last bin is the X-ray test source's energy).  Returns
    both paths (the second None without energy arrays)."""
    import os
    n = len(shells["N_PASSED"])
    flux = shells["SUM_WEIGHTS"]
    total = float(flux.sum())
    p1 = os.path.join(outpath, "shell_breakdown_%s.csv" % year)
    with open(p1, "w") as f:
        f.write("shell,coating,R1 [mm],selected,hit nickel,passed till window,passed,flux,flux error,flux fraction\n")
        for s in range(n):
            f.write("%d,%d,%.17g,%d,%d,%d,%d,%.17g,%.17g,%.17g\n" % (
                s, int(shells["coating"][s]), float(shells["R1"][s]), int(shells["N_SELECTED"][s]), int(shells["N_HIT_NICKEL"][s]),
                int(shells["N_PASSED_TILL_WINDOW"][s]), int(shells["N_PASSED"][s]), float(flux[s]), float(np.sqrt(shells["SUM_WEIGHTS_SQ"][s])),
                float(flux[s]) / total if total > 0 else 0.0))
    p2 = None
    if "energy_counts" in shells:
        p2 = os.path.join(outpath, "energies_by_shell_%s.csv" % year)
        e = np.append(np.asarray(energies, dtype=np.float64), np.nan)   # index n_energies: the X-ray test source's energy
        with open(p2, "w") as f:
            f.write("shell,energy index,energy [keV],rays,flux\n")
            for s in range(n):
                for k in np.nonzero(shells["energy_counts"][s])[0]:
                    f.write("%d,%d,%.17g,%d,%.17g\n" % (s, k, e[k], int(shells["energy_counts"][s][k]), float(shells["energy_weights"][s][k])))
    return p1, p2


channel_block_len = _lib.channel_block_len
split_channels = _lib.split_channels
origin_block_len = _lib.origin_block_len
split_origin = _lib.split_origin
aperture_block_len = _lib.aperture_block_len
split_aperture = _lib.split_aperture

# Which coupling every term of the emission table carries (csrc/sart_emission.hip: the g_ae^2, g_agamma^2 and g_anuclei^2 factors of
# its eight terms, in the order of _lib.EM_TERMS), and the reference values the library's table is made with (readOpacityFile.nim:640-643).
COUPLINGS = ("g_ae", "g_agamma", "g_anuclei")
TERM_COUPLING = dict(compton="g_ae", term1="g_ae", ee_brems="g_ae", free_free="g_ae", primakoff="g_agamma", long_plasmon="g_agamma",
                     trans_plasmon="g_agamma", iron57="g_anuclei")
REFERENCE_COUPLINGS = dict(g_ae=1e-13, g_agamma=1e-12, g_anuclei=1e-15)


def group_emission_components(components, grouping: str):
    """(rates [T][nR][nE], names, couplings) from the eight components of emission_table: ``"terms"`` keeps them, ``"couplings"``
    sums them per coupling of TERM_COUPLING (numpy sums, in term order)."""
    comp = np.asarray(components, dtype=np.float64)
    assert comp.shape[0] == len(_lib.EM_TERMS)
    if grouping == "terms":
        return comp, list(_lib.EM_TERMS), [TERM_COUPLING[t] for t in _lib.EM_TERMS]
    if grouping == "couplings":
        rates = np.zeros((len(COUPLINGS),) + comp.shape[1:])
        for k, term in enumerate(_lib.EM_TERMS):
            rates[COUPLINGS.index(TERM_COUPLING[term])] += comp[k]
        return rates, list(COUPLINGS), list(COUPLINGS)
    raise ValueError("grouping must be \"terms\" or \"couplings\", not %r" % (grouping,))


def coupling_signal(channels: dict, g_ae: float | None = None, g_agamma: float | None = None, g_anuclei: float | None = None,
                    ref: dict | None = None) -> dict:
    """The expected signal at other couplings from ONE trace_channels result: sum_t s_t X_t with s_t = (g_t / g_t,ref)^2 for the
    flux, the energy spectrum and the image (those that ``channels`` holds).  ``channels["couplings"]`` names the coupling of every
    channel; ``ref`` the couplings the emission table was made with (default REFERENCE_COUPLINGS); a coupling left None stays at its
    reference.  ``flux_error`` is the bound sum_t s_t sqrt(sum w^2_t): the channels share their rays, so their errors are fully
    correlated and add linearly (triangle inequality) - the exact error sqrt(sum_rays (sum_t s_t c_t)^2) is never larger.
    This rescales the EMISSION only: the conversion in the magnet carries its own g_agamma^2, which belongs to the setup."""
    ref = dict(REFERENCE_COUPLINGS, **(ref or {}))
    g = dict(g_ae=g_ae, g_agamma=g_agamma, g_anuclei=g_anuclei)
    if channels.get("couplings") is None:
        raise ValueError("coupling_signal: the channels carry no coupling names (set_source_channels(..., couplings=...))")
    scale = np.array([1.0 if g[c] is None else (float(g[c]) / ref[c]) ** 2 for c in channels["couplings"]])
    out = {"scale": scale, "flux": float(np.dot(scale, channels["SUM_WEIGHTS"])),
           "flux_error": float(np.dot(scale, np.sqrt(channels["SUM_WEIGHTS_SQ"])))}
    if "energy_weights" in channels:
        out["energy_weights"] = np.tensordot(scale, channels["energy_weights"], axes=1)
    if "images" in channels:
        out["image"] = np.tensordot(scale, channels["images"], axes=1)
    return out


def write_channel_csvs(outpath: str, year: str, channels: dict, energies: np.ndarray, chip_max: float, r_sigma1: float = 0.0,
                       r_sigma2: float = 0.0):
    """`flux_by_channel_{year}.csv` (channel, name, contributing rays, flux, its Monte-Carlo error, its fraction of the channels' sum),
    with energy arrays `energies_by_channel_{year}.csv` (flux per channel and energy bin) and with images one
    `axion_image_{year}_{name}.csv` per channel (write_image_csv with the chip's width ``chip_max`` and the containment radii of
    the whole image).  Returns the list of paths."""
    import os
    names = channels["names"]
    flux = np.asarray(channels["SUM_WEIGHTS"], dtype=np.float64)
    total = float(flux.sum())
    paths = [os.path.join(outpath, "flux_by_channel_%s.csv" % year)]
    with open(paths[0], "w") as f:
        f.write("channel,name,contributing rays,flux,flux error,flux fraction\n")
        for t, name in enumerate(names):
            f.write("%d,%s,%d,%.17g,%.17g,%.17g\n" % (t, name, int(channels["N_CONTRIBUTING"][t]), float(flux[t]),
                                                     float(np.sqrt(channels["SUM_WEIGHTS_SQ"][t])), float(flux[t]) / total if total > 0 else 0.0))
    if "energy_weights" in channels:
        paths.append(os.path.join(outpath, "energies_by_channel_%s.csv" % year))
        e = np.append(np.asarray(energies, dtype=np.float64), np.nan)
        with open(paths[-1], "w") as f:
            f.write("channel,name,energy index,energy [keV],flux\n")
            for t, name in enumerate(names):
                for k in np.nonzero(channels["energy_weights"][t])[0]:
                    f.write("%d,%s,%d,%.17g,%.17g\n" % (t, name, k, e[k], float(channels["energy_weights"][t][k])))
    if "images" in channels:
        for t, name in enumerate(names):
            paths.append(os.path.join(outpath, "axion_image_%s_%s.csv" % (year, name)))
            write_image_csv(paths[-1], channels["images"][t], float(chip_max), r_sigma1, r_sigma2)
    return paths


def read_flux_by_channel_csv(path: str) -> dict:
    """The columns of a flux_by_channel_{year}.csv, keyed by the header (``name`` as a list of strings, the rest as arrays)."""
    with open(path) as f:
        header = f.readline().strip().split(",")
        rows = [line.strip().split(",") for line in f if line.strip()]
    return {h: ([r[i] for r in rows] if h == "name" else np.array([float(r[i]) for r in rows])) for i, h in enumerate(header)}


def read_shell_breakdown_csv(path: str) -> dict:
    """The columns of a shell_breakdown_{year}.csv as arrays, keyed by the header."""
    with open(path) as f:
        header = f.readline().strip().split(",")
    data = np.loadtxt(path, delimiter=",", skiprows=1, ndmin=2)
    return {h: data[:, i] for i, h in enumerate(header)}


def containment_radii(spectra: dict):
    """rSigma1, rSigma2 (unweighted) and rSigma1W, rSigma2W (weighted) of generateResultPlots (raytracer.nim:2459-2527)."""
    host = _lib.load_host()
    r = [C.c_double() for _ in range(4)]
    rc, rw = np.ascontiguousarray(spectra["radial_counts"]), np.ascontiguousarray(spectra["radial_weights"])
    _lib.check(host.sart_host_containment_radii(_lib.as_dp(rc), _lib.as_dp(rw), rc.size, spectra["radial_max"],
                                                *[C.byref(x) for x in r]), host=True)
    return tuple(x.value for x in r)


def write_image_csv(path: str, image: np.ndarray, chip_max: float, r_sigma1: float, r_sigma2: float) -> float:
    """plotHeatmap's `axion_image_{year}{suffix}.csv` (raytracer.nim:887-921).  Returns the total flux."""
    host = _lib.load_host()
    img = np.ascontiguousarray(image, dtype=np.float64)
    flux = C.c_double()
    _lib.check(host.sart_host_write_image_csv(path.encode(), _lib.as_dp(img), img.shape[0], chip_max, r_sigma1, r_sigma2,
                                              C.byref(flux)), host=True)
    return flux.value


def accumulator_len(image_n: int = 256) -> int:
    return image_n * image_n + _lib.SART_ACC_COUNT


def mass_scan_len(n_masses: int) -> int:
    """sart_mass_scan_len: 8-byte slots of a scan accumulator."""
    return (int(n_masses) + 1) * _lib.SCAN_ROW


def split_mass_scan(acc: np.ndarray, n_masses: int):
    """(per-mass dict of arrays, shared-counter dict) from a finalized scan accumulator."""
    rows = np.asarray(acc, dtype=np.float64).reshape(n_masses + 1, _lib.SCAN_ROW)
    per_mass = {k: rows[:n_masses, i].copy() for k, i in _lib.SCAN.items()}
    shared = {k: float(rows[n_masses, i]) for k, i in _lib.SCAN_SHARED.items()}
    return per_mass, shared


def split_mass_scan_spectra(spec: np.ndarray, n_masses: int, n_bands: int) -> dict:
    """Dict of ``SUM_WEIGHTS`` / ``SUM_WEIGHTS_SQ`` [n_masses][n_bands + 1] and ``N_ON_DETECTOR`` [n_bands + 1] from a finalized
    spectra buffer of a banded mass scan (the last cell of each row: everything outside the window)."""
    cells = np.asarray(spec, dtype=np.float64).reshape(n_masses + 1, n_bands + 1, _lib.MSPEC_CELL)
    out = {k: cells[:n_masses, :, i].copy() for k, i in _lib.MSPEC.items()}
    out["N_ON_DETECTOR"] = cells[n_masses, :, _lib.MSPEC_COUNTS["N_ON_DETECTOR"]].copy()
    return out


def band_of_energy_index(e_idx, bands) -> np.ndarray:
    """The cell of a banded mass scan that energy index ``e_idx`` (array) belongs to: (e - e0) // width inside the window
    [e0, e0 + n_bands width), n_bands (the outside cell) otherwise - the rule of include/sart.h, in numpy."""
    e0, width, n_bands = (int(v) for v in bands)
    e = np.asarray(e_idx, dtype=np.int64)
    inside = (e >= e0) & (e < e0 + n_bands * width)
    return np.where(inside, (e - e0) // width, n_bands).astype(np.int64)


def energy_bands(energies, e_min_kev: float, e_max_kev: float, n_bands: int):
    """Bands of a banded mass scan from a request in keV.  ``energies``: the context's energy table (FullSetup.energies), a uniform
    grid of points with step dE; index e stands for the cell [energies[e] - dE / 2, energies[e] + dE / 2).  Returns
    ((e0, width, n_bands), edges in keV [n_bands + 1]).  ValueError for a request the index grid cannot represent: e_min_kev must
    be a cell edge, (e_max_kev - e_min_kev) / n_bands a whole number >= 1 of cells, the window inside the table, n_bands in
    [1, 31]."""
    en = np.asarray(energies, dtype=np.float64)
    if en.ndim != 1 or en.size < 2:
        raise ValueError("energy_bands: the energy table needs at least two points")
    step = (en[-1] - en[0]) / (en.size - 1)
    if not step > 0 or np.abs(np.diff(en) - step).max() > 1e-9 * step:
        raise ValueError("energy_bands: the energy table is not a uniform grid")
    if not 1 <= int(n_bands) <= _lib.MSPEC_MAX_BANDS or int(n_bands) != n_bands:
        raise ValueError("energy_bands: n_bands must be a whole number in [1, %d]" % _lib.MSPEC_MAX_BANDS)
    n_bands = int(n_bands)
    if not (np.isfinite(e_min_kev) and np.isfinite(e_max_kev) and e_max_kev > e_min_kev):
        raise ValueError("energy_bands: needs finite e_min_kev < e_max_kev")
    lo = en[0] - 0.5 * step                    # lower edge of cell 0
    f0 = (e_min_kev - lo) / step
    fw = (e_max_kev - e_min_kev) / (step * n_bands)
    e0, width = int(round(f0)), int(round(fw))
    if abs(f0 - e0) > 1e-6 or abs(fw - width) > 1e-6:
        raise ValueError("energy_bands: [%r, %r] keV in %d bands is not a whole number of energy cells (cell edges at %r + k x %r keV)"
                         % (float(e_min_kev), float(e_max_kev), n_bands, float(lo), float(step)))
    if e0 < 0 or width < 1 or e0 + n_bands * width > en.size:
        raise ValueError("energy_bands: the window leaves the energy table ([%r, %r] keV)" % (float(lo), float(lo + step * en.size)))
    return (e0, width, n_bands), lo + step * (e0 + width * np.arange(n_bands + 1))


def angular_scan_len(n_angles: int) -> int:
    """sart_angular_scan_len: 8-byte slots of an angular-scan accumulator."""
    return (int(n_angles) + 1) * _lib.ASCAN_ROW


def split_angular_scan(acc: np.ndarray, n_angles: int):
    """(per-angle dict of arrays, shared-counter dict) from a finalized angular-scan accumulator."""
    rows = np.asarray(acc, dtype=np.float64).reshape(n_angles + 1, _lib.ASCAN_ROW)
    per_angle = {k: rows[:n_angles, i].copy() for k, i in _lib.ASCAN.items()}
    shared = {k: float(rows[n_angles, i]) for k, i in _lib.ASCAN_SHARED.items()}
    return per_angle, shared


def split_image_blocks(blocks: np.ndarray, image_n: int, n_radial_bins: int, n_e1: int, radial_max: float = 10.0):
    """(images [K, ny, nx], K summary dicts, K split_spectra dicts or None) from K finalized accumulator blocks of
    image_n x image_n pixels (n_radial_bins = 0: without spectra)."""
    blocks = np.asarray(blocks, dtype=np.float64)
    n_img = image_n * image_n
    images = blocks[:, :n_img].reshape(-1, image_n, image_n).copy()
    summaries = [{k: float(b[n_img + i]) for k, i in _lib.ACC.items()} for b in blocks]
    spectra = [split_spectra(b[n_img + _lib.SART_ACC_COUNT:], n_radial_bins, n_e1, radial_max) for b in blocks] if n_radial_bins else None
    return images, summaries, spectra


def angle_image_names(year: str, angles) -> list:
    """File names of the per-angle images of an angular scan: `axion_image_{year}_angle_{a:.2f}.csv` as plotHeatmap's suffix
    (raytracer.nim:2787) writes them.  Where two angles give the same name at two decimals, every name takes the fewest decimals
    (up to 17) that make them distinct; angles that are equal to the last bit keep that name with `_{k}` (their index) behind it."""
    angles = [float(a) for a in angles]
    values = set(angles)
    d = next((d for d in range(2, 18) if len({"%.*f" % (d, a) for a in values}) == len(values)), 17)
    tags = ["%.*f" % (d, a) for a in angles]
    counts = {}
    for t in tags:
        counts[t] = counts.get(t, 0) + 1
    return ["axion_image_%s_angle_%s%s.csv" % (year, t, "_%d" % k if counts[t] > 1 else "") for k, t in enumerate(tags)]


def calculateFluxFractions(tracer: RayTracer, n_rays: int = 1_000_000, seed: int = 299792458,
                           ray_id_offset: int = 0, shells: bool = False):
    """calculateFluxFractions (raytracer.nim:2755-2776) in histogram form: NumberOfPointsSun rays ->
    256x256 focal-plane image (heatmaptable2, :2629) + counters (:2252-2257) + total flux (:885).  ``shells``: the same trace
    with the per-shell breakdown (RayTracer.trace_shells): (image, summary, spectra, shells)."""
    if shells:
        return tracer.trace_shells(n_rays, seed, ray_id_offset)
    return tracer.trace_histogram(n_rays, seed, ray_id_offset)


def performAxionMassScan(tracer: RayTracer, masses_ev, n_rays_per_mass: int = 1_000_000, seed: int = 299792458,
                         flags: int | None = None, ray_id_offset: int = 0, errors: bool = False, bands=None):
    """m_a scan (BASELINE configs[4]) through the C++ host driver: flux (sum of weights) per axion mass.  Gas stage: the
    fused scan kernel - every ray of [ray_id_offset, ray_id_offset + n_rays_per_mass) is traced once and weighed for every
    mass (common random numbers).  ``errors``: also return sqrt(sum of squared weights) and the passed-ray counts.
    ``bands`` = (e0, width, n_bands) (energy_bands()): the banded scan (gas stage only) - returns a dict with ``flux``, ``sigma``,
    ``n_passed`` per mass, the per-mass spectra ``band_flux`` and ``band_sigma`` = sqrt(sum of squared weights)
    [n_masses][n_bands + 1] (last cell: outside the window) and ``band_counts`` [n_bands + 1], the rays per band on the detector."""
    host = _lib.load_host()
    masses = np.ascontiguousarray(masses_ev, dtype=np.float64)
    fluxes, sq, n_pass = np.empty_like(masses), np.empty_like(masses), np.empty_like(masses)
    fl = tracer.full.flags if flags is None else flags
    if bands is not None:
        e0, width, n_bands = (int(v) for v in bands)
        cells = max(n_bands, 0) + 1
        bf, bsq, bn = np.empty((masses.size, cells)), np.empty((masses.size, cells)), np.empty(cells)
        _lib.check(host.sart_host_axion_mass_scan_spectra(tracer.handle, _lib.as_dp(masses), masses.size, n_rays_per_mass, seed,
                                                          ray_id_offset, fl, e0, width, n_bands, _lib.as_dp(fluxes), _lib.as_dp(sq),
                                                          _lib.as_dp(n_pass), _lib.as_dp(bf), _lib.as_dp(bsq), _lib.as_dp(bn)), host=True)
        return dict(flux=fluxes, sigma=np.sqrt(sq), n_passed=n_pass, band_flux=bf, band_sigma=np.sqrt(bsq), band_counts=bn)
    _lib.check(host.sart_host_axion_mass_scan(tracer.handle, _lib.as_dp(masses), masses.size, n_rays_per_mass, seed,
                                              ray_id_offset, fl, _lib.as_dp(fluxes), _lib.as_dp(sq), _lib.as_dp(n_pass)), host=True)
    return (fluxes, np.sqrt(sq), n_pass) if errors else fluxes


def performAxionMassScanHostLoop(tracer: RayTracer, masses_ev, n_rays_per_mass: int = 1_000_000, seed: int = 299792458,
                                 flags: int | None = None, ray_id_offset: int = 0, same_rays: bool = True):
    """The reference-shaped scan (a host loop: set the mass, re-trace, sum) - what the fused kernel replaces; kept as the
    comparison of the parity tests and of bench.py.  ``same_rays``: every mass on the same ray ids (what the fused scan
    computes), else mass i on its own block of ids = the C++ host driver sart_host_perform_axion_mass_scan."""
    masses = np.ascontiguousarray(masses_ev, dtype=np.float64)
    out = np.empty_like(masses)
    if not same_rays:
        host = _lib.load_host()
        fl = tracer.full.flags if flags is None else flags
        _lib.check(host.sart_host_perform_axion_mass_scan(tracer.handle, _lib.as_dp(masses), masses.size, n_rays_per_mass, seed,
                                                          ray_id_offset, fl, _lib.as_dp(out)), host=True)
        return out
    m0 = tracer.full.setup.m_axion
    try:
        for i, m in enumerate(masses):
            tracer.set_axion_mass(float(m))
            off = ray_id_offset + (0 if same_rays else i * n_rays_per_mass)
            out[i] = tracer.trace_histogram(n_rays_per_mass, seed, off, flags)[1]["SUM_WEIGHTS"]
    finally:
        tracer.set_axion_mass(m0)
    return out


def performEnergyScan(tracer: RayTracer, energies_kev, n_rays: int = 1_000_000, seed: int = 299792458, flags: int | None = None,
                      ray_id_offset: int = 0) -> dict:
    """Detection efficiency - and, for a parallel beam, the effective area - of the X-ray test source as a function of its
    energy, through the fused energy scan (sart_trace_energy_scan: every ray traced once and weighed at every energy, the same
    rays for all energies).  Returns a dict of arrays: ``energies`` [keV], ``sum_weights``, ``sigma`` = sqrt(sum of squared
    weights), ``n_passed``, ``efficiency`` = sum_weights / N_RAYS and ``effective_area_cm2`` = pi (test_radius / 10)^2 x efficiency
    when the source is a parallel beam (None otherwise: a point source's efficiency is no area), plus ``shared`` (the
    energy-independent counters)."""
    energies = np.ascontiguousarray(energies_kev, dtype=np.float64)
    rows, shared = tracer.trace_energy_scan(energies, n_rays, seed, ray_id_offset, flags)
    n = shared["N_RAYS"]
    eff = rows["SUM_WEIGHTS"] / n if n > 0 else np.full(energies.size, np.nan)
    cur = _lib.Setup()
    _lib.check(tracer.lib.sart_get_setup(tracer.handle, C.byref(cur)))
    area = np.pi * (cur.test_radius / 10.0) ** 2 * eff if cur.test_parallel else None
    return dict(energies=energies, sum_weights=rows["SUM_WEIGHTS"], sigma=np.sqrt(rows["SUM_WEIGHTS_SQ"]), n_passed=rows["N_PASSED"],
                efficiency=eff, effective_area_cm2=area, shared=shared)


def performAngularScan(tracer: RayTracer, angularScanMin: float, angularScanMax: float, numAngularScanPoints: int = 50,
                       n_rays_per_angle: int = 1_000_000, seed: int = 299792458, flags: int | None = None,
                       angles=None, ray_id_offset: int = 0, fused: bool = False, errors: bool = False, images: bool = False):
    """performAngularScan (raytracer.nim:2778-2802) through the C++ host driver: returns (angles, fluxes,
    relative fluxes).  ``angles`` overrides the linspace (used when angle bins are sharded over GPUs).
    ``fused = False``: the reference's shape - a host loop, angle i on its own block of fresh ray ids (flux-only launches).
    ``fused = True``: the fused scan kernel - every ray of [ray_id_offset, ray_id_offset + n_rays_per_angle) is sampled once
    and turned through every angle (common random numbers); with ``errors`` also sqrt(sum of squared weights) and the
    passed-ray counts.
    ``images``: every angle's full result set as well (the per-angle calculateFluxFractions of :2787), appended to the tuple as
    (images [K, 256, 256], K summary dicts, K spectra dicts) - fused: sart_trace_angular_scan_images; host loop: one trace_spectra
    launch per angle on the ids the flux-only host loop uses (the fluxes then come from those launches)."""
    host = _lib.load_host()
    angles = np.linspace(angularScanMin, angularScanMax, numAngularScanPoints) if angles is None else \
        np.ascontiguousarray(angles, dtype=np.float64)
    if images:
        return _angular_scan_images(tracer, angles, n_rays_per_angle, seed, flags, ray_id_offset, fused, errors)
    fluxes = np.empty_like(angles)
    rel = np.empty_like(angles)
    fl = tracer.full.flags if flags is None else flags
    if fused:
        sq, n_pass = np.empty_like(angles), np.empty_like(angles)
        _lib.check(host.sart_host_angular_scan(tracer.handle, _lib.as_dp(angles), angles.size, n_rays_per_angle, seed, ray_id_offset,
                                               fl, _lib.as_dp(fluxes), _lib.as_dp(rel), _lib.as_dp(sq), _lib.as_dp(n_pass)), host=True)
        return (angles, fluxes, rel, np.sqrt(sq), n_pass) if errors else (angles, fluxes, rel)
    _lib.check(host.sart_host_perform_angular_scan(tracer.handle, _lib.as_dp(angles), angles.size, n_rays_per_angle,
                                                   seed, ray_id_offset, fl, _lib.as_dp(fluxes), _lib.as_dp(rel)), host=True)
    return angles, fluxes, rel


def _angular_scan_images(tracer: RayTracer, angles: np.ndarray, n_rays: int, seed: int, flags, ray_id_offset: int, fused: bool,
                         errors: bool):
    if fused:
        imgs, summ, spec, (rows, _) = tracer.trace_angular_scan_images(angles, n_rays, seed, ray_id_offset, flags, spectra=True)
        fluxes = rows["SUM_WEIGHTS"]
        extra = (np.sqrt(rows["SUM_WEIGHTS_SQ"]), rows["N_PASSED"]) if errors else ()
    else:
        cur = _lib.Setup()
        _lib.check(tracer.lib.sart_get_setup(tracer.handle, C.byref(cur)))
        ty0 = cur.telescope_turned_y_deg   # put back on every way out, as the host driver does
        imgs, summ, spec = [], [], []
        try:
            for i, a in enumerate(angles):   # raytracer.nim:2791-2800, the ray ids of sart_host_perform_angular_scan
                tracer.set_telescope_angles(turned_y_deg=float(a))
                img, s, sp = tracer.trace_spectra(n_rays, seed, ray_id_offset + i * n_rays, flags)
                imgs.append(img)
                summ.append(s)
                spec.append(sp)
        finally:
            tracer.set_telescope_angles(turned_y_deg=ty0)
        imgs = np.stack(imgs) if imgs else np.empty((0, 256, 256))
        fluxes = np.array([s["SUM_WEIGHTS"] for s in summ])
        extra = (np.full(angles.size, np.nan), np.array([s["N_PASSED"] for s in summ])) if errors else ()
    return (angles, fluxes, fluxes / fluxes.max()) + extra + ((imgs, summ, spec),)
