// sart_device.h — PODs shared by the host side of libsart (sart_api.hip) and the gfx950 kernels
// (sart_kernels.hip).  Everything here is *derived* from sart_setup_t + the tables by the hoist_*
// functions of sart_api.hip: per-setup / per-shell / per-energy-index constants are evaluated once on
// the host with the reference's formulas (cited there) so that the per-ray kernel contains no
// setup-only transcendental.
//
// Where the data lives on the device:
//   DevParams        by value in the kernel arguments (scalar registers; loop-invariant)
//   ShellDev[], shell LUT, fluxRadiusCDF + its guide table
//                    HBM -> staged into LDS once per workgroup (coalesced loads)
//   diffFluxCDFs (23.6 MB), its guide table, EnergyDev[], reflectivity (12 MB / coating)
//                    HBM, served by L2 / Infinity Cache (random, dependent gathers)
#pragma once
#include <stdint.h>

namespace sart {

constexpr int kMaxShells = 64;
constexpr int kMaxStrips = 16;       // half the number of window strips that are looped over
constexpr int kRadiusGuide = 2048;   // buckets of the guide table in front of fluxRadiusCDF
// The CDF's entries crowd towards 1 (the outer radii emit next to nothing): uniform buckets of 1/2048 hold up to hundreds of them
// there, and a wave with ONE such lane walks a binary search.  u >= 31/32 therefore has a second guide of 1024 buckets of 1/32768
// behind the first: entries 0 .. 2048 = lowerBound(cdf, k / 2048), entries 2049 .. 3073 = lowerBound(cdf, 31/32 + j / 32768).
// With K = floor(u 2^32) (Uniforms::u2_hi): bucket K >> 21, or 2049 + ((K - kRadiusGuideTopStart) >> 17) for K >= kRadiusGuideTopStart.
constexpr int kRadiusGuideTop = 1024;
constexpr uint32_t kRadiusGuideTopStart = 0xF8000000u;   // 31/32 of 2^32
constexpr int kRadiusGuideEntries = kRadiusGuide + 1 + kRadiusGuideTop + 1;   // 3074
// Guide table in front of every row of diffFluxCDFs (lowerBound of the energy draw, raytracer.nim:464-468).  Buckets in the
// uniform u of the draw: width 1/kEnergyGuideDiv below u = 31/32; above, where a solar spectrum's CDF creeps towards 1 over hundreds
// of energies, buckets of constant RELATIVE width in v = 1 - u (64 per octave of v, read off the bits of the double v) down
// to v = 2^-30.  A bucket then holds 0-2 table entries almost everywhere, and the draw resolves with ONE gather of four
// consecutive CDF values instead of a data-dependent binary search (a chain of dependent HBM / Infinity-Cache round trips).
// 1024 rather than 2048 uniform buckets: the guide shrinks from 14.1 to 10.2 MB (its hot part from 2 to 1 MB per 500 radius
// rows) while a bucket still holds fewer than four entries wherever the CDF rises; measured -1.3 % on CAST / LLNL, -1 % on
// BabyIAXO, 512 buckets: no further gain (profiles/r03_exp_guide_density.txt).  Results do not depend on the density.
#ifndef SART_ENERGY_GUIDE_DIV
#define SART_ENERGY_GUIDE_DIV 1024
#endif
constexpr int kEnergyGuideDiv = SART_ENERGY_GUIDE_DIV;    // uniform buckets per unit of u (a power of two)
constexpr int kEnergyGuideUniform = kEnergyGuideDiv / 32 * 31;   // buckets [k / Div, (k + 1) / Div), k < Div * 31/32
constexpr int kEnergyGuideLogMax = 25 * 64;               // log buckets j = 1 .. 1600 (j = 0: the single point u = 31/32)
constexpr int kEnergyGuideBuckets = kEnergyGuideUniform + kEnergyGuideLogMax + 1;
constexpr int kEnergyGuideEntries = kEnergyGuideBuckets + 1;   // u16 per row: bucket k is bracketed by entries k, k + 1
constexpr uint32_t kEnergyGuideCode0 = (1023u - 5u) << 6;  // (high word of the double 1/32) >> 14
// Bucket records of the energy draw (HotB::energy_records; built by energy_records_kernel, sart_tables.hip): one 16-byte record per
// (radius row, guide bucket) that holds the bucket's guide entry `lo` and the first kEnergyRecordK entries of cdf_hi32 inside the
// bucket, so that ONE gather settles a word-exact draw (energy_draw_finish): lo + #{thresholds below the word}.  Every bucket's
// words lie in one aligned block of 2^22 once the words of the log buckets are taken one lower (bucket j there is the words 2^32 - m
// of an aligned block of m: it starts one past an aligned address), so a threshold keeps its low 22 bits:
//   word s < 4:  t[s] << 10 | ten bits: {lo[0:10) | lo[10] << 8, t[4][14:22) | t[4][6:14) | mark << 8, t[4][0:6) << 2}
// (the low bytes of words 1 - 3, in that order, are the upper 22 bits of t[4] << 10: two v_perm_b32 put the fifth threshold into the
// form of the other four, which need no extraction at all - a word whose upper 22 bits are t compares like t << 10)
// with t[s] = cdf_hi32[lo + s] - off - block (off = 0 uniform, 1 log), kEnergyRecordEmpty where the bucket holds no such entry or the
// entry is not below the bucket's last word, and mark = "more than kEnergyRecordK entries inside".  lo counts the entries of the
// bracket that lie below the bucket's first word in (log buckets: the guide takes an upper bound of the edge below).
constexpr int kEnergyRecordK = 5;
constexpr uint32_t kEnergyRecordEmpty = 0x3FFFFFu;
constexpr int kEnergyRecordMaxEnergies = 2047;            // lo has 11 bits: larger tables keep the two-level draw
constexpr int kEnergyCdfPad = 4;                          // 1.0-valued pad behind every CDF row (four-wide candidate gather)
constexpr int kShellLutMax = 1024;   // cells of the radial look-up table of the shell selection
constexpr int kMaxRadii = 2048;      // fluxRadiusCDF entries that fit the LDS stage
constexpr int kSinCosEntries = 129;  // (cos, sin)(pi k / 64), k = 0 .. 128: table behind the sampling angles

// Per-shell constants (Wolter-I pair j).  Quadratics are expressed in the telescope frame with
// the ray parametrised by z:  X(z) = X0 + sx z,  Y(z) = Y0 + sy z, so that with
//   A = sx^2 + sy^2,  D = X0 sx + Y0 sy,  Q = X0^2 + Y0^2
// a = A - k,  half_b = D + hb,  c = Q - cc   (findPosCone/Parabolic/Hyperbolic, raytracer.nim:628-729).
struct ShellDev {
  double r1;        // allR1[j]
  double r1_outer;  // allR1[j] + allThickness[j]
  // mirror 1 (cone, angle beta | paraboloid)
  double m1_k, m1_hb, m1_cc, m1_zhi;   // z range (0, m1_zhi)
  // mirror 2 (cone r4, angle 3 beta | hyperboloid)
  double m2_k, m2_hb, m2_cc, m2_zlo, m2_zhi;
  double m2_rc;     // cone 2: radius at z = m2_zlo (r4)
  // surface normals (calcNormalVec, raytracer.nim:731-759)
  double n1_tan;    // cone: tan(beta)
  double n1_r3t;    // paraboloid: r3 * tan(beta);    n1_r3sq = r3^2, n1_e = 2 r3 tan(beta)
  double n1_r3sq, n1_e;
  double n2_tan;    // cone: tan(3 beta)
  double n2_r3t;    // hyperboloid: r3 * tan(3 beta); n2_r3sq = r3^2, n2_e = 2 r3 tan(3 beta)
  double n2_r3sq, n2_e, n2_invF;       // invF = 1 / (f + r3 cot(2 beta))
  // detector distance for this shell (raytracer.nim:2070-2072), already divided by cos(pipe angle)
  double dist_det, dist_det_end;
  double dist_det_raw;                 // distDet before the 1/cos (xray-test straight-through, :2131)
  // lineHitsNickel (raytracer.nim:1722): r1 - (R1[j-1] + t[j-1]); unused for j == 0
  double nickel_num;
  // reflectivity grid of this shell: layers.lowerBound(j) (raytracer.nim:1573)
  int32_t coating;
  int32_t refl_row0;   // coating * (n_energies + 1): first row of this shell's grid in refl[][n_angles]
};
static_assert(sizeof(ShellDev) % 8 == 0, "ShellDev is staged into LDS as 8-byte words");

// Per-energy-index constants: the energy of a ray is one of the n_energies table values
// (raytracer.nim:470-471: energies[idx], clamped to >= 0.03 keV), so every E-only factor is a table.
// Row n_energies holds the same quantities for the X-ray test source's fixed energy (:1771).
struct EnergyDev {
  double energy;       // max(0.03, energies[idx])
  double t_window;     // windowTransmission.eval(E)      (:2179)
  double t_strongback; // strongbackTransmission.eval(E)  (:2170)
  double a_gas;        // gasAbsorption.eval(E)           (:2190)
  // gas stage (axionMassforMagnet.nim:75-113)
  double gamma;        // Gamma(E) in eV
  double inv_two_e_ev; // 1 / (2 * E[eV])  (momentumTransfer, :68: q = |m_gamma^2 - m_a^2| / (2 E), as a multiplication)
  double mu_pipe;      // massAtt * rhoPipe   * 100   [1/m]
  double mu_magnet;    // massAtt * rhoMagnet * 100   [1/m]
};

// Loop-invariant scalars, passed by value as a kernel argument.
struct DevParams {
  // ---- sampling (raytracer.nim:412-471) ----
  double sun_distance, sun_radius;
  double radius_cb, radius_cb_sq, length_b, length_coldbore;
  double pipe1_len, pipe2_len, pipe1_radius_sq;
  int32_t n_radii, n_energies;
  int32_t radius_span;        // max entries of fluxRadiusCDF between two guide marks a draw can meet (informational: the kernel reads four
                              // candidates and searches on only in a wider bracket)
  int32_t lut_n;              // cells of the shell selection's look-up table (here: its slot beside lut_inv_step holds mirror_miss_radius)
  // ---- X-ray test source (raytracer.nim:1765-1806) ----
  int32_t test_active, test_parallel;
  double test_x, test_y, test_z, test_radius, test_radius_sq, test_collimator_z;
  // ---- telescope frame (raytracer.nim:1878-1899) ----
  int32_t telescope_wolter;   // 1: paraboloid + hyperboloid (XMM, Abrixas); 0: cones (LLNL)
  int32_t telescope_kind;     // SART_TK_*
  int32_t n_shells, rotated;
  double l_mirror;
  double rx_c, rx_s, ry_c, ry_s, half_length_telescope;
  double entrance_x, entrance_y;
  // ---- shell selection (raytracer.nim:1932-1957) ----
  double r1_last;             // allR1[^1]
  double lut_inv_step;
  // The mirror-miss shortcut of trace_histogram_kernel.  A ray whose radial distance at the entrance plane lies above
  // mirror_miss_radius selects a shell for which the host has proved two things (sart_api.hip: mirror_miss_bounds_of): (a) if the ray
  // at z = l_mirror is more than kMirrorMissEps (mm^2, squared distances from the axis) inside the first mirror's radius there,
  // pick_root accepts neither root of the mirror's quadratic; (b) if its squared slope tsx^2 + tsy^2 is below mirror_miss_slope_sq,
  // the nickel test of a ray that missed the first mirror is true.  The kernel makes those compares in phase A and ends such a ray
  // there with +1 in N_HIT_NICKEL, which is all phase B would have made of it.  Radius +infinity: the shortcut is off.  (Two floats,
  // rounded to the safe side, in the eight bytes the block has to spare.)
  float mirror_miss_radius, mirror_miss_slope_sq;
  // A ray that selects the innermost shell (none below it, so no nickel test, :1719) from a radial distance below this value
  // provably stays inside that shell's first mirror over its whole length: neither root of findPosParabolic lies in the
  // mirror (:677-682), the input point comes back and the ray ends at the no-hit test (:2055) with every counter untouched.
  // Phase A counts it as "shell selected" and does not hand it to phase B.  -1: not proved for this setup (sart_api.hip:
  // shell0_miss_radius_of).
  double shell0_miss_radius;
  // ---- opaque structures (raytracer.nim:1635-1704) ----
  double spider_z;            // -85 (XMM) / -35 (Abrixas)
  double inner_radius;        // XMM: 64.7 (<=) ; Abrixas: 37.5 (<)
  double ring_lo, ring_hi;    // XMM: 130.7 .. 151.6 (exclusive)
  // spokes every 360/spoke_n degrees, half width w:  blocked <=> cos(spoke_n phi) >= cos(spoke_n w)
  int32_t spoke_n;            // 16 (XMM: 22.5 deg) | 6 (Abrixas: 60 deg)
  int32_t inner_blocks;       // XMM: 1 if the hole loop always blocks (htNone), -1: evaluate it
  double spoke_cos_thr;
  int32_t hole_type, number_of_holes;
  double hole_in_optics;
  // ---- detector plane (raytracer.nim:797-814, 2133-2204) ----
  double pipe_c, pipe_s, d_cb_xray;
  double lateral_shift, transversal_shift;
  double radius_window_sq, chip_cx, chip_cy;
  double theta_c, theta_s;
  int32_t n_half_strips, stage_gas;
  double strip_lo[kMaxStrips], strip_hi[kMaxStrips];
  // ---- weights (raytracer.nim:363-365, 1582-1625, 2207-2212) ----
  double conv_k;              // P(a->gamma) = conv_k * pathCB^2 (vacuum)
  double exposure;            // 3.585e3*3600*1.5*90 | 9.5e6*3600*12*90
  double gas_m_gamma_sq, gas_term1, gas_inv_hbarc_m;   // m_gamma^2, (g B / 2)^2, 1e-3 / 1.97e-7 (mm -> 1/eV)
  // |m_gamma^2 - m_a^2| (one IEEE subtraction of the two squares; the mass scan's table holds the same expression per mass).
  // (Takes the place of m_a^2 in this block: the LDS copy of the blob keeps its size, and with it the rings their addresses -
  // 16 bytes more and every ring access needs an extra address add, +2 vector instructions per loop iteration.)
  double gas_dm2_abs;
  // ---- reflectivity (raytracer.nim:1533-1580) ----
  int32_t refl_n_angles, n_coatings;
  double refl_angle_min, refl_inv_dangle, refl_dangle;
};
static_assert(sizeof(DevParams) < 2048, "DevParams travels in the kernel-argument segment");

// The few scalars phase A touches for every ray: by value in the kernel arguments (SGPRs).
struct HotA {
  double sun_distance, sun_radius;
  double radius_cb, radius_cb_sq, length_b, length_coldbore;
  double dz1, dz2, dz3;        // z of cold-bore exit / pipe exits relative to the magnetic-field exit plane
  double pipe1_radius_sq;
  double entrance_x, entrance_y;
  double r1_last, lut_inv_step;
  double spider_z, spoke_cos_thr, inner_radius, ring_lo, ring_hi;
  int32_t test_active, rotated, telescope_kind, spoke_n;
  // radial_table: 1 if the look-up table in LDS holds the cells of the radial verdict table (RadialLds; sart_api.hip:
  // build_radial_table), 0 if it holds the shell selection's own cells (today's compares).  Wave-uniform switch of the solar-source
  // histogram kernels.  (In the slot of the informational radius_span, which no kernel read: the argument block keeps its layout.)
  int32_t n_shells, lut_n, radial_table, inner_blocks;
  // Stage A0 (early rejection on the bore-exit radius alone): the hi word w of the uniform u3 that sets the
  // radius of the point on the bore exit (r = R sqrt(u3), raytracer.nim:418) lies in zone z if
  // zone_lo[z] <= w <= zone_hi[z]; rays in a zone provably die before the mirrors.  Bit z of zone_reached:
  // they provably pass bore + pipes first (they still count as "reached the telescope").  0 zones: stage off.
  // Bit kA0WideBit + p of zone_reached (kA0WideMask: p = 0 and 2, the even passes): in pass p the histogram kernels' loop takes two
  // words of the stream in one iteration where ring 0 has room (sart_trace_histogram.inc: the wide pass; sart_api.hip:
  // a0_wide_rule decides it per setup).  In this word because the loop reads it once per pass anyway: the switch costs the
  // kernels no register and no load.
  int32_t n_zones;
  uint32_t zone_reached;
  uint32_t zone_lo[4], zone_hi[4];
};
constexpr int kMaxZones = 4;
constexpr int kA0WideBit = 8;
constexpr uint32_t kA0WideMask = 0x5u << kA0WideBit;
static_assert(kA0WideBit >= kMaxZones, "the wide-pass switch lies above the zones' bits");

// What phase B needs as *scalars* at its gathers: the bases of the HBM-resident tables and the sizes their offsets are
// built from.  Passed by value as a kernel argument and re-read with scalar loads at the start of a phase-B pass, so
// that every gather is `global_load ... v_offset32, s[base]` instead of 64-bit vector address arithmetic on pointers
// fetched from LDS.  All tables are < 4 GB (checked on the host), offsets are 32-bit.
struct HotB {
  const double* diff_flux_cdfs;       // [n_radii][cdf_stride]: every row followed by kEnergyCdfPad entries of 1.0
  // The same table as the upper 32 of the 52 bits of floor(cdf * 2^52), same stride: what the four-candidate count of the energy
  // draw gathers (16 bytes instead of 32; half the cache footprint of the table that competes hardest for L2).  The draw's
  // uniform is k * 2^-52 with an integer k, so  cdf[i] < u  <=>  floor(cdf[i] 2^52) < k, and the upper 32 bits decide that unless
  // they are equal (one draw in ~1e9): then, and in buckets wider than four entries, the f64 row decides.
  const uint32_t* cdf_hi32;
  const uint16_t* energy_guide;       // [n_radii][kEnergyGuideEntries]
  const EnergyDev* energy_tab;        // [n_energies + 1]
  const double* refl;                 // [n_coatings][n_energies + 1][n_angles]
  int32_t n_energies, refl_n_angles;
  int32_t cdf_stride;                 // n_energies + kEnergyCdfPad
  int32_t records_on;                 // 1: energy_records holds the bucket records and the word-exact draw goes through them
  // [n_radii][kEnergyGuideBuckets][4]: the bucket records of the word-exact draw (above); null (and records_on = 0): the two-level
  // draw (tables of more than kEnergyRecordMaxEnergies energies, SART_ENERGY_RECORDS=0)
  const uint32_t* energy_records;
};

// ---- the folded form of the histogram kernel (sart_kernels.hip: HistCfg, folded_histogram_kernel; variants 7 / 8) ----
// The constant-path variants 5 / 6 compiled with the answers of the reference's default configuration as constants: the values
// below, and `true` for every member of FoldInputs.  A launch takes the folded form only when folded_form_applies() - the one
// place that says so on the host - and the kernel's configuration type folds exactly these answers.
constexpr int kFoldedSpokes = 16;          // the XMM spider (hoist_setup)
constexpr int kFoldedHalfStrips = 2;       // number_of_strips = 4: every shipped detector setup
// launch flags whose tests are folded (all clear in the folded form)
constexpr uint32_t kFoldedFlags = 1u << 0 | 1u << 1 | 1u << 2 | 1u << 3 | 1u << 4;   // SART_CF_IGNORE_DET_WINDOW .. SART_CF_XRAY_TEST
struct FoldInputs {
  // the context
  bool constant_path;     // hist_variant_of says 5 or 6 (solar source, no hole loop, telescope not turned, constant path)
  bool records_on;        // HotB::records_on: the energy draw goes through the bucket records
  bool radial_table;      // HotA::radial_table
  bool zones;             // HotA::n_zones > 0 (stage A0 runs)
  bool xmm;               // SART_TK_XMM: Wolter optics with the ring and the 16-spoke spider
  int spoke_n;            // HotA::spoke_n
  int n_half_strips;      // DevParams::n_half_strips
  // the launch
  uint32_t flags;         // sart_trace_params_t::flags
  bool spectra;           // sart_trace_params_t::spectra
  // the knob
  bool no_folded;         // SART_NO_FOLDED
};
inline bool folded_form_applies(const FoldInputs& f) {
  return f.constant_path && f.records_on && f.radial_table && f.zones && f.xmm && f.spoke_n == kFoldedSpokes &&
         f.n_half_strips == kFoldedHalfStrips && (f.flags & kFoldedFlags) == 0u && !f.spectra && !f.no_folded;
}

// Device pointers of one context.
struct DevTables {
  const double* sincos_tab;           // [kSinCosEntries][2]: (cos, sin)(pi k / 64), correctly rounded
  const ShellDev* shells;             // [n_shells]
  const uint8_t* shell_lut;           // [lut_n]: first shell with R1 > k * lut_step
  const double* flux_radius_cdf;      // [n_radii]
  const uint16_t* radius_guide;       // [kRadiusGuide + 1]
  const double* diff_flux_cdfs;       // [n_radii][n_energies + kEnergyCdfPad] (rows padded with 1.0)
  const uint16_t* energy_guide;       // [n_radii][kEnergyGuideEntries]
  const EnergyDev* energy_tab;        // [n_energies + 1]
  // reflectivity re-tabulated per energy index: refl[coating][e_idx][angle] (see hoist_reflectivity)
  const double* refl;                 // [n_coatings][n_energies + 1][n_angles]
};

// DevParams + DevTables as one blob in HBM; staged into LDS by every workgroup.
struct DevBlob {
  DevParams P;
  DevTables T;
};
static_assert(sizeof(DevBlob) % 8 == 0, "DevBlob is staged into LDS as 8-byte words");

constexpr int kMaxImageReplicas = 128;   // power of two

struct TraceArgs {
  uint64_t n_rays, ray_id_offset;
  // Image atomics go to replica (wave id & replica_mask) of a scratch image: contended f64 atomics on a small
  // focal spot serialise at the memory side.  fold_replicas_kernel adds the replicas into the caller's
  // accumulator.  replica_mask = 0 (wide images): `replicas` is the accumulator itself, no fold.
  double* replicas;
  uint32_t replica_mask;
  uint32_t replica_stride;   // doubles between two replicas (image size + padding, see sart_api.hip)
  // Per-workgroup partial sums of the SART_ACC_COUNT scalars (plain stores; fold_scalars_kernel adds them to the
  // accumulator): thousands of f64 atomics on the same 11 addresses serialise for hundreds of microseconds.
  double* partials;
  uint32_t seed_lo, seed_hi;
  uint32_t flags;
  int32_t image_nx, image_ny;
  double image_x_min, image_y_min, image_inv_step_x, image_inv_step_y;
  // optional spectra behind the scalars (include/sart.h: sart_accumulator_len_spectra)
  int32_t spectra, n_radial_bins;
  double radial_inv_bin;
  // Image tile in LDS: pixels [tile_x0, tile_x0 + tile_n) x [tile_y0, tile_y0 + tile_n) are accumulated per workgroup with
  // ds_add_f64 and flushed once at the end of the kernel; everything else goes to global atomics.  tile_n = 0: off.  Pixel
  // (tx, ty) of the tile is cell tile_base + ty tile_n + tx of the tile space (cells 0 .. kTileRingCells - 1: ring 0, free when stage
  // A0 is off, or ring 1's path column in the constant-path variants; kTileExtraCells more behind the tables): tile_base = 0 and
  // tile_n <= kImageTileMax when the ring cells are free, else tile_base = kTileRingCells and tile_n <= kImageTileExtraMax.
  int32_t tile_x0, tile_y0, tile_n, tile_base;
  // SART_ACCUM_FIXED64 (include/sart.h "accumulation mode"): 1 / quantum of the weights and of the squared weights (powers
  // of two); positions use kFixedPositionScale, the reflectivity spectrum kFixedReflectScale.  Unused by the f64 kernels.
  double fx_scale_w, fx_scale_w2;
};
// Fused axion-mass scan (include/sart.h: sart_trace_mass_scan): phase B evaluates the gas-stage conversion probability of every
// surviving ray for the masses of this table and accumulates per mass.  One launch takes up to kScanMaxMasses masses: their
// accumulators ([mass][sum of w, sum of w^2][kScanLanes] f64 or int64 = 512 B per mass; lanes l and l + 32 of a wave share a cell) live
// in the 16 KB of LDS that the image tile uses in the histogram kernels (a scan accumulates no image).
constexpr int kScanMaxMasses = 32;
constexpr int kScanLanes = 32;
struct ScanMass {
  double dm2_abs;                 // |m_gamma^2 - m_a^2| in eV^2 (host: the same IEEE subtraction the single-mass kernel performs)
  double fx_scale_w, fx_scale_w2; // SART_ACCUM_FIXED64: 1 / quantum of the weights and of the squared weights of THIS mass
  // Two spare words per entry.  The banded scan (include/sart.h: sart_trace_mass_scan_spectra) keeps its band table in those of the
  // first two entries - the argument block keeps its size, and with it the code of every kernel that shares it: m[0].aux = {band_e0,
  // band_mul}, m[1].aux = {band_window, 0}.  The cell index of the accumulators means "energy band" there: band = (e - band_e0) / width
  // for (uint32_t)(e - band_e0) < band_window = n_bands width, else the outside cell n_bands; the division is
  // __umulhi(2 d + 1, band_mul) with band_mul = ceil(2^31 / width), which the host checks against d / width for every d an energy
  // index of the context can give (sart_api.hip: bands_prepare).  Zero in every other launch.
  uint32_t aux[2];
};
struct ScanArgs {
  int32_t n_masses;               // masses of this launch (<= kScanMaxMasses); 0 in every launch that is not a scan
  int32_t n_bands;                // banded scan: its bands (1 .. kScanBandsMax); 0 in every other launch
  // [n_blocks][kScanMaxMasses][4] per-workgroup {sum w, sum w^2, rays whose weight vanishes for this mass only, 0}; banded scan: behind
  // them [n_blocks][kScanMaxMasses + 1][2 kScanLanes], a workgroup's cells per mass, then its per-band counts
  double* partials;
  ScanMass m[kScanMaxMasses];
};
static_assert(sizeof(ScanMass) == 32 && offsetof(ScanMass, aux) == 24 && sizeof(ScanArgs) == 16 + 32 * kScanMaxMasses,
              "the kernel re-reads ScanArgs with scalar loads at these offsets");
constexpr int kScanPartialSlots = 4;
constexpr int kScanBandSlots = (kScanMaxMasses + 1) * 2 * kScanLanes;   // banded scan: partial slots of one workgroup behind the plain ones
constexpr int kScanBandsMax = kScanLanes - 1;   // bands of a banded scan: the 32 cells of a mass less the outside cell

// Fused angular scan (include/sart.h: sart_trace_angular_scan): the telescope's angles enter a ray at the transformation into the
// telescope's frame (raytracer.nim:1878-1899) and nowhere before it, so trace_angular_scan_kernel samples a ray and takes it through
// bore and pipes ONCE and runs telescope frame -> opaque structures -> shell selection -> mirrors -> weight once per angle of this
// table.  One launch takes up to kAScanMaxAngles angles: per angle a workgroup keeps [sum of w, sum of w^2][kScanLanes] f64 / int64
// cells - in the u5 column of ring 1, which this kernel does not use (the energy draw happens in front of the angle loop: the ring
// carries the energy index) - and four counters in LDS.
constexpr int kAScanMaxAngles = 32;
struct AScanAngle {
  // rotateInY(rotateInX(., turnedX), turnedY) about (0, 0, lT/2) as hoist_setup() evaluates it for this angle (TelRot)
  double rx_c, rx_s, ry_c, ry_s, half_length_telescope;
  double shell0_miss_radius;      // DevParams::shell0_miss_radius of this angle (the bound follows the tilt)
  // third column of the rotation: mx = rx_s, my = -(rx_c ry_s), mz = rx_c ry_c - what phase B needs to find z of pointExitCB in
  // the rotated frame (staged into LDS: a phase-B pass holds rays of several angles)
  double mx, my, mz;
  double _pad;
};
struct AScanArgs {
  int32_t n_angles, _pad;         // angles of this launch (1 .. kAScanMaxAngles)
  double* partials;               // [n_blocks][kAScanMaxAngles][kAScanPartialSlots] per-workgroup sums (plain stores; fold_ascan_kernel adds them)
  AScanAngle a[kAScanMaxAngles];
};
static_assert(sizeof(AScanAngle) == 80 && sizeof(AScanArgs) == 16 + 80 * kAScanMaxAngles, "the kernel re-reads AScanArgs with scalar loads at these offsets");
// per-workgroup partial row of one angle: sum w, sum w^2, N_PASSED, N_HIT_NICKEL, N_PASSED_TILL_WINDOW, N_SHELL_SELECTED,
// (angle 0 only) N_REACHED_TELESCOPE of the workgroup, unused
constexpr int kAScanPartialSlots = 8;

// Fused energy scan (include/sart.h: sart_trace_energy_scan): with the X-ray test source the energy is a constant of the setup
// (raytracer.nim:1771) that enters a ray's weight only, so trace_energy_scan_kernel traces every ray ONCE and forms its weight for
// every energy of this table.  One launch takes up to kEScanMaxEnergies energies: what the weight needs of energy k (the E-only
// factors of its EnergyDev row, hoisted by the host exactly as row n_energies of the single launch) travels here and is read with
// scalar loads; the reflectivity rows of the scan are a table of their own ([n_coatings][row_stride][n_angles], `refl`).  Per energy
// a workgroup keeps [sum of w, sum of w^2][kScanLanes] f64 / int64 cells in ring 0's space (the test source runs no stage A0) and two
// counters in LDS.
constexpr int kEScanMaxEnergies = 32;
struct EScanEnergy {
  double t_window, t_strongback, a_gas;           // EnergyDev of this energy
  double gamma, inv_two_e_ev, mu_pipe, mu_magnet;
  double fx_scale_w, fx_scale_w2;                 // SART_ACCUM_FIXED64: 1 / quantum of the weights and squared weights of THIS energy
  double _pad;
};
struct EScanArgs {
  int32_t n_energies;             // energies of this launch (1 .. kEScanMaxEnergies)
  int32_t row_stride;             // energies of the scan's reflectivity table (rows per coating)
  double* partials;               // [n_blocks][kEScanMaxEnergies][kScanPartialSlots] {sum w, sum w^2, N_PASSED, N_PASSED_TILL_WINDOW}
  const double* refl;             // first row of this launch's energies in the scan's reflectivity table (coating 0)
  double _pad;
  EScanEnergy e[kEScanMaxEnergies];
};
static_assert(sizeof(EScanEnergy) == 80 && sizeof(EScanArgs) == 32 + 80 * kEScanMaxEnergies, "the kernel re-reads EScanArgs with scalar loads at these offsets");

constexpr double kFixedPositionScale = 4294967296.0;        // 2^32 per mm
constexpr double kFixedReflectScale = 1099511627776.0;      // 2^40
constexpr int kFixedLimbBits = 40;                          // two-limb sums: value = hi * 2^40 + lo
// LDS image tile of the histogram kernels: 16 waves x 128 doubles of ring space (ring 0, or ring 1's path column) + kTileExtraCells
// doubles behind the tables: what the radius CDF leaves free in LDS as 32-bit words and the end of the 160 KB (kRingExtraCells, all
// that the kernels whose rings are WaveRings have there), and 512 bytes per wave that ring 1 of the histogram kernels does not need
// (HistRings: the energy draw's uniform travels as its 32-bit word), less the radial verdict table: 63 x 63 <= 2048 + 1922 cells
// Radial verdict table of the solar-source histogram kernels: everything phase A decides from the radial distance at the entrance
// plane alone (inner disc, XMM ring, beyond the last shell, shell selection, glass front, the two sure-miss radii) is a piecewise
// constant function of it.  Entry k: breakpoint b[k] and a word of three verdict bytes - just below b[k], exactly at it, just above
// it; a byte is code << 6 | shell with code 0 not selected, 1 selected and below shell0_miss_radius, 2 selected, 3 selected and
// above mirror_miss_radius.  The look-up table's cell of a ray gives the index of the first breakpoint whose own cell is not lower
// (kRadialMarked: several breakpoints in that cell, or cell 0, where an unordered radial distance lands - such lanes evaluate the
// compares).  The table takes kRadialTableCells of the cells behind the tables from the image tile.
constexpr int kRadialMax = 128;
constexpr int kRadialMarked = 255;
struct RadialLds {
  double b[kRadialMax];
  uint32_t w[kRadialMax];
};
constexpr int kRadialTableCells = (int)(sizeof(RadialLds) / 8);
// the device buffer behind DevTables::shell_lut: the shell selection's cells, the verdict table's cells, the table
constexpr int kRadialCellsOffset = kShellLutMax, kRadialTableOffset = 2 * kShellLutMax;
constexpr int kTileRingCells = 2048;
constexpr int kRingExtraCells = 1090;
constexpr int kTileExtraCells = 1922;
static_assert(kTileExtraCells == kRingExtraCells + 16 * 512 / 8 - kRadialTableCells, "16 waves x 512 bytes, less the radial verdict table");
// Margin of the end-radius compare of the mirror-miss shortcut, mm^2 (DevParams::mirror_miss_radius; the host checks per shell that it
// is more than 1e4 times what rounding can move either side by)
constexpr double kMirrorMissEps = 1e-3;
constexpr int kImageTileMax = 63;
constexpr int kImageTileExtraMax = 43;   // 43 x 43 <= kTileExtraCells: the tile of the variants whose rings are all in use

// The four breakdowns of the histogram trace, per shell, per emission channel, per cell of the solar table and per cell of the
// entrance plane, are one pipeline: breakdown_histogram_body (sart_kernels.hip) is the generic histogram kernel with a per-workgroup
// table in LDS, and shell_histogram_kernel, channel_histogram_kernel, origin_histogram_kernel and aperture_histogram_kernel are its
// users (ShellBreakdown / ChannelBreakdown / OriginBreakdown / ApertureBreakdown: the argument struct, the table, its cells).  What
// follows is what each of them keeps in that table and hands to its fold.
//
// Per-shell breakdown of the histogram trace (include/sart.h: sart_trace_histogram_shells_device).  shell_histogram_kernel keeps,
// per workgroup and shell, four u32 counters and two sums in LDS - in the last kShellTableCells cells behind the tables, where the
// histogram kernels keep the end of the image tile (its tile is therefore at most kShellImageTileMax / kShellImageTileExtraMax wide)
// - and stores them once to partials[n_blocks][kMaxShells][kShellPartialSlots]; fold_shells_kernel adds those to the caller's block.
constexpr int kShellPartialSlots = 6;   // N_SELECTED, N_HIT_NICKEL, N_PASSED_TILL_WINDOW, N_PASSED, sum of w, sum of w^2
constexpr int kShellTableCells = kMaxShells * 4 / 2 + kMaxShells * 2;   // the u32 counters and the 8-byte sums, in 8-byte cells
constexpr int kShellImageTileMax = 53;        // 53 x 53 <= kTileRingCells + kRingExtraCells - kShellTableCells
constexpr int kShellImageTileExtraMax = 28;   // 28 x 28 <= kRingExtraCells - kShellTableCells
struct ShellArgs {
  double* block;          // the caller's block: rows of SART_SHELL_ROW slots, then (spectra) the per-shell energy counts and weights
  double* partials;       // [n_blocks][kMaxShells][kShellPartialSlots] per-workgroup counters and sums (plain stores)
  int32_t n_shells, n_energies1;
  double _pad;
};
static_assert(sizeof(ShellArgs) == 32, "the kernel re-reads ShellArgs with scalar loads");

// Emission-channel breakdown of the histogram trace (include/sart.h: sart_trace_histogram_channels_device).  channel_histogram_kernel
// keeps, per workgroup and channel, three sums - of c = w f, of c^2, of c outside the image - spread over kChanLanes cells each (lane l
// adds to cell l % kChanLanes: passed rays of one wave do not all meet in one LDS address) and one u32 counter spread likewise, in the last
// kChanTableCells cells behind the tables (as the shell table: its image tile is at most kChanImageTileMax / kChanImageTileExtraMax
// wide), and stores their sums once to partials[n_blocks][kMaxChannels][kChanPartialSlots]; fold_channels_kernel adds those to the
// caller's block.  Per-channel energy bins and pixels take global atomics.
constexpr int kMaxChannels = 8;
constexpr int kChanLanes = 16;
constexpr int kChanPartialSlots = 4;   // sum of c, sum of c^2, sum of c outside the image, N_CONTRIBUTING
constexpr int kChanTableCells = kMaxChannels * 3 * kChanLanes + kMaxChannels * kChanLanes / 2;   // the sums and the u32 counters, in 8-byte cells
constexpr int kChanImageTileMax = 51;        // 51 x 51 <= kTileRingCells + kRingExtraCells - kChanTableCells
constexpr int kChanImageTileExtraMax = 25;   // 25 x 25 <= kRingExtraCells - kChanTableCells
static_assert(kChanImageTileMax * kChanImageTileMax <= kTileRingCells + kRingExtraCells - kChanTableCells &&
                  kChanImageTileExtraMax * kChanImageTileExtraMax <= kRingExtraCells - kChanTableCells,
              "the channel kernel's image tile leaves the channel table alone");
struct ChannelArgs {
  double* block;          // the caller's block: rows of SART_CHAN_ROW slots, then (spectra) energy_weights[T][n_energies1], then T images
  double* partials;       // [n_blocks][kMaxChannels][kChanPartialSlots] per-workgroup sums and counters (plain stores)
  const double* frac;     // [n_radii][n_energies][stride]: the fractions of the ray drawn at (r, e), padded with 0
  int32_t n_channels, stride;       // T in [1, kMaxChannels]; T rounded up to 1, 2, 4 or 8
  int32_t n_radii, n_energies;      // the table's shape (the gather clamps its indices to it)
  int32_t n_energies1, _pad;
};
static_assert(sizeof(ChannelArgs) == 48, "the kernel re-reads ChannelArgs with scalar loads");

// Solar-origin map of the histogram trace (include/sart.h: sart_trace_histogram_origin_device).  origin_histogram_kernel adds every
// passed ray to the cell (r_idx, e_idx) it was drawn in - three global atomics into one 32-byte cell of the caller's block: the map
// has millions of cells, so no replicas and no LDS staging - and keeps, per workgroup and wave, the head's three sums (N_PASSED, sum
// of w, sum of w^2: the wave's own scalars) in the last kOriginTableCells cells behind the tables (its image tile is therefore at most
// kOriginImageTileMax / kOriginImageTileExtraMax wide), stored once to partials[n_blocks][kOriginPartialSlots]; fold_origin_kernel adds
// those to the head of the caller's block.
constexpr int kOriginPartialSlots = 4;   // N_PASSED, sum of w, sum of w^2, unused
constexpr int kOriginTableCells = 16 * kOriginPartialSlots;   // one row per wave of a 1024-thread workgroup
constexpr int kOriginImageTileMax = 55;        // 55 x 55 <= kTileRingCells + kRingExtraCells - kOriginTableCells
constexpr int kOriginImageTileExtraMax = 32;   // 32 x 32 <= kRingExtraCells - kOriginTableCells
static_assert(kOriginImageTileMax * kOriginImageTileMax <= kTileRingCells + kRingExtraCells - kOriginTableCells &&
                  (kOriginImageTileMax + 1) * (kOriginImageTileMax + 1) > kTileRingCells + kRingExtraCells - kOriginTableCells &&
                  kOriginImageTileExtraMax * kOriginImageTileExtraMax <= kRingExtraCells - kOriginTableCells &&
                  (kOriginImageTileExtraMax + 1) * (kOriginImageTileExtraMax + 1) > kRingExtraCells - kOriginTableCells,
              "the origin kernel's image tile is the largest square that leaves its table alone");
struct OriginArgs {
  double* block;          // the caller's block: SART_ORIGIN_HEAD slots, then cells[n_radii][n_energies][SART_ORIGIN_CELL]
  double* partials;       // [n_blocks][kOriginPartialSlots] per-workgroup sums (plain stores)
  int32_t n_radii, n_energies;   // the map's shape (the kernel clamps its indices to it)
  double _pad;
};
static_assert(sizeof(OriginArgs) == 32, "the kernel re-reads OriginArgs with scalar loads");

// Aperture map of the histogram trace (include/sart.h: sart_trace_histogram_aperture_device).  aperture_histogram_kernel adds every
// passed ray to the cell of a grid over the entrance plane that its entrance point (X0, Y0: pointEntranceXRT) falls in, or to the one
// cell behind the grid where it falls outside the window - the origin map's three global atomics into one 32-byte cell - and keeps the
// origin kernel's head table: the same per-wave rows, the same partials, the same image tile maxima, fold_origin_kernel.
constexpr int kAperturePartialSlots = kOriginPartialSlots;
constexpr int kApertureTableCells = kOriginTableCells;
constexpr int kApertureImageTileMax = kOriginImageTileMax;
constexpr int kApertureImageTileExtraMax = kOriginImageTileExtraMax;
constexpr int kApertureMaxSide = 4096;        // nx, ny in [1, kApertureMaxSide]
constexpr int kApertureMaxCells = 1 << 22;    // nx ny <= kApertureMaxCells: a cell index is 32-bit, a byte offset below 2^28
struct ApertureArgs {
  double* block;          // the caller's block: SART_APERTURE_HEAD slots, then cells[ny][nx][SART_APERTURE_CELL], then the outside cell
  double* partials;       // [n_blocks][kAperturePartialSlots] per-workgroup sums (plain stores)
  int32_t nx, ny;         // the grid's shape
  double x_min, inv_step_x, y_min, inv_step_y;   // cell of a point: ((X0 - x_min) inv_step_x, (Y0 - y_min) inv_step_y), inv_step = n / (max - min)
  double _pad;
};
static_assert(sizeof(ApertureArgs) == 64, "the kernel re-reads ApertureArgs with scalar loads");

}  // namespace sart
