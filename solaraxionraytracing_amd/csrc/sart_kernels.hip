// sart_kernels.hip — gfx950 (MI355X, CDNA4) kernels of the per-ray hot path.
//
// One ray per lane, f64 throughout (the Sun sits 1.5e14 mm away and the mirror quadratics cancel
// ~1e5-magnitude terms).  The algorithm is the reference's `traceAxion`
// (src/raytracer.nim:1736-2221), restructured for the device:
//   * every per-setup / per-shell / per-energy-index quantity is a table built on the host
//     (sart_api.hip: hoist_*), so the kernel has no setup-only transcendental;
//   * the straight line through bore and pipes is carried as (point on the bore exit, slopes
//     dx/dz, dy/dz) instead of differences of 1e11-magnitude points: same geometry, without the
//     reference's ~1e-5 mm cancellation noise;
//   * mirror hits use the cancellation-free form of the same quadratic roots; the reflection
//     v cos2a - (v x axis) sin2a (:778-779) is evaluated algebraically (no asin/sin/cos), and on a
//     hit the surface normals reduce to closed forms without a square root;
//   * a Philox4x32-7 counter block per ray (key = seed, counter = global ray id) replaces the
//     reference's shared xoroshiro stream, draw order as in the reference;
//   * the path is split where most rays die (bore, pipes, spider, glass fronts: ~2/3 of all rays for
//     BabyIAXO) into three stages that each run on full waves: A0 (one Philox block: rays that the
//     radius of their bore-exit point alone proves dead), A1 = phase A (sample + cuts + shell
//     selection), B = phase B (mirrors + weights + accumulation); survivors are compacted with a
//     wavefront ballot + prefix count into per-wave LDS rings between the stages;
//   * phase A's scalars travel in the kernel arguments (re-read with scalar loads at the start of
//     each pass); the radius CDF, its guide table, the shell table and the shell look-up table
//     are staged into LDS once per workgroup;
//   * results are accumulated on the device: f64 atomics into the focal-plane image, wave
//     reductions for the scalars.
// Lines cited as ":NNNN" refer to src/raytracer.nim of the reference.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <type_traits>

#include "../../include/sart.h"
#include "sart_device.h"
#include "sart_math.h"

namespace sart {

// ------------------------------------------------------------------------------------------------
// Philox4x32-7 (Salmon et al., SC'11: seven rounds are the fewest that pass BigCrush; ten are the paper's default with margin).
// Round 6 went from ten rounds and two blocks per ray to seven rounds and one block per ray (uniforms_of): the counter RNG was a
// quarter of the ray kernel's vector instructions, and v_mad_u64_u32 is not a full-rate one.  The stream is a free parameter of
// the path (the reference draws from xoroshiro128+; parity with it is statistical, tests/test_gpu_parity.py: independent streams).
// ------------------------------------------------------------------------------------------------
struct U4 { uint32_t x, y, z, w; };
constexpr int kPhiloxRounds = 7;

__device__ __forceinline__ U4 philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                         uint32_t k1) {
#pragma unroll
  for (int r = 0; r < kPhiloxRounds; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;   // one v_mad_u64_u32 yields both halves
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
    const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    // a ^ b ^ c in ONE instruction: gfx950's v_bitop3_b32 with the truth table of the three-input xor (0x96); the compiler
    // does not form it from two `^` by itself (it emits two v_xor_b32)
    const uint32_t n0 = __builtin_amdgcn_bitop3_b32(hi1, c1, k0, 0x96);
    const uint32_t n2 = __builtin_amdgcn_bitop3_b32(hi0, c3, k1, 0x96);
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return U4{c0, c1, c2, c3};
}

// Word n of the shared word stream behind the high word of u3: word (n & 3) of the Philox block with counter
// (n >> 2, 3, 0).  Four consecutive ray ids share one block (stage A0 computes it once per lane for four rays).
__device__ __forceinline__ U4 stream_block(uint64_t group, uint32_t k0, uint32_t k1) {
  return philox4x32((uint32_t)group, (uint32_t)(group >> 32), 3u, 0u, k0, k1);
}
__device__ __forceinline__ uint32_t word_of(const U4& b, uint32_t k) {
  return k == 0u ? b.x : (k == 1u ? b.y : (k == 2u ? b.z : b.w));
}

// Assembly comment at the head of a pipeline stage: tools/isa_histogram.py attributes the instructions of the compiler's
// listing to stages by these markers.  No instruction, no operands, no clobbers.
#define SART_STAGE_MARK(name) asm volatile("; SART_STAGE " name)

// Lane mask of a predicate.  HIP's __ballot() materialises the predicate as 0 / 1 and compares again (two VALU
// instructions); the builtin takes the compare's lane mask as it is.
__device__ __forceinline__ uint64_t ballot64(bool pred) { return __builtin_amdgcn_ballot_w64(pred); }

// A compile-time f64 constant in a scalar register pair.  LLVM otherwise materialises a polynomial coefficient with two
// v_mov_b32 into the destination of a two-address v_fmac_f64 (three vector instructions per Horner step instead of
// one); s_mov_b32 issues on the scalar unit beside other waves' vector instructions.  `volatile` keeps the moves next to
// their use (hoisted out of the persistent loop the registers would be spilled through VGPR lanes).
template <uint64_t BITS>
__device__ __forceinline__ double scalar_const() {
  uint32_t lo, hi;
  asm volatile("s_mov_b32 %0, %2\n\ts_mov_b32 %1, %3" : "=s"(lo), "=s"(hi) : "n"((uint32_t)BITS), "n"((uint32_t)(BITS >> 32)));
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | (uint64_t)lo));
}
#define SC(x) (scalar_const<__builtin_bit_cast(uint64_t, (double)(x))>())

// One Horner step p x + C with the coefficient C as a scalar operand: v_fma_f64 v, v, v, s.  Left to itself LLVM selects the
// two-address v_fmac_f64 for a single-use addend and copies the constant into the destination first (two v_mov_b32 per
// step, also when the constant already sits in scalar registers).
// HORNER hands the coefficient to the "s" operand as a plain constant: the COMPILER then writes the two s_mov_b32, as
// instructions it knows.  (They used to come from scalar_const's own asm statement.  The hazard recogniser treats every
// register an asm statement defines as if a forwarding-hazard instruction had written it, and counts the asm statements
// between that definition and its first vector reader as zero wait states: each step carried an s_nop between the moves and
// the FMA, four issue slots for one FMA.  A compiler-written s_mov_b32 needs none - the hardware interlocks a scalar write
// against a vector read - and it counts as the wait state between the FMAs of two steps.)  Constants are materialised per basic
// block at instruction selection, and MachineLICM is off for this file (Makefile): nothing hoists them out of the persistent
// loop, and within a block equal coefficients are merged - two chains of one polynomial written step by step side by side
// (asin_small_pair, spoke_measure_pair) share one pair of moves per coefficient.
__device__ __forceinline__ double fma_vvs(double p, double x, double c_scalar) {
  double r;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(p), "v"(x), "s"(c_scalar));
  return r;
}
#define HORNER(p, x, c) fma_vvs((p), (x), (double)(c))

// Uniform in [0, 1) from two words (hi word first): 52 random mantissa bits under the exponent of 1.0,
// minus 1.0 — the construction of Nim's std/random rand(1.0) (and of the oracle).
__device__ __forceinline__ double u52(uint32_t hi, uint32_t lo) {
  // 0x3FF0000000000000 | ((hi:lo) >> 12) as two funnel shifts (v_alignbit_b32): low word = (hi:lo) >> 12, high word =
  // (0x3FF:hi) >> 12 = 0x3FF00000 | (hi >> 12)
  const uint32_t mlo = __builtin_amdgcn_alignbit(hi, lo, 12u);
  const uint32_t mhi = __builtin_amdgcn_alignbit(0x3FFu, hi, 12u);
  return __longlong_as_double((long long)(((uint64_t)mhi << 32) | (uint64_t)mlo)) - 1.0;
}

// ------------------------------------------------------------------------------------------------
// small math helpers
// ------------------------------------------------------------------------------------------------
// sin and cos of pi a, a = TURNS * u for u in [0, 1) (TURNS = 2: a full turn, 1: half a turn), to <= ~1.5 ulp:
// k = rint(64 a), r = a - k / 64 exactly (|r| <= 1/128), (C, S) = (cos, sin)(pi k / 64) from the 129-entry table in LDS
// (correctly rounded on the host, exact zeros and ones at the multiples of pi/2), short Taylor polynomials in r
// (truncation < 4e-17 relative for |pi r| <= pi/128) and the angle-addition formulas.  No quadrant selects, and 7
// polynomial coefficients (scalar registers, shared by the three evaluations of a ray) instead of 16.
struct SinCosCoef { double s3, s2, s1, s0, d3, d2, d1; };   // sin(pi r) = r (s0 + y (s1 + y (s2 + y s3))), cos(pi r) = 1 + y (d1 + ...)
__device__ __forceinline__ SinCosCoef sincos_coef() {
  return SinCosCoef{SC(-0.5992645293207921), SC(2.5501640398773455), SC(-5.16771278004997), SC(3.141592653589793),
                    SC(-1.3352627688545895), SC(4.0587121264167685), SC(-4.934802200544679)};
}
template <int TURNS>
__device__ __forceinline__ void sincos_turns(double u, const double* __restrict__ table, const SinCosCoef& K, double* sn, double* cs) {
  constexpr double T = (double)TURNS;
  const double kf = __builtin_rint(u * (64.0 * T));          // 0 .. 64 TURNS
  const double r = fma(-1.0 / 64.0, kf, u * T);              // T u - k / 64, exact (T is a power of two)
  const double2 t = reinterpret_cast<const double2*>(table)[(int)kf];   // one ds_read_b128: (C, S)
  const double x = r * r;
  const double sr = fma(fma(fma(K.s3, x, K.s2), x, K.s1), x, K.s0) * r;
  const double cr = fma(fma(fma(K.d3, x, K.d2), x, K.d1), x, 1.0);
  *sn = fma(t.x, sr, t.y * cr);                               // sin(a + b) = S cr + C sr
  *cs = fma(-t.y, sr, t.x * cr);                              // cos(a + b) = C cr - S sr
}

// asin for the grazing angles of the path (|x| < ~0.03): odd Taylor series
// asin x = x + x^3/6 + 3x^5/40 + 5x^7/112 + 35x^9/1152 + 63x^11/2816 + 231x^13/13312 + 143x^15/10240,
// truncation error < 1e-19 below 0.06; the library function outside.
// The series is evaluated unconditionally (straight-line code the scheduler can interleave with its surroundings); the
// library call is a divergent alternative that a wave skips when no lane needs it.
__device__ __forceinline__ double asin_small(double x, double x2) {   // x2 = x^2 (the caller has it)
  double p = 0.01396484375;                        // 143/10240
  p = HORNER(p, x2, 0.017352764423076924);         // 231/13312
  p = HORNER(p, x2, 0.022372159090909092);         // 63/2816
  p = HORNER(p, x2, 0.030381944444444444);         // 35/1152
  p = HORNER(p, x2, 0.044642857142857144);         // 5/112
  p = HORNER(p, x2, 0.075);                        // 3/40
  p = HORNER(p, x2, 0.16666666666666666);          // 1/6
  double r = fma(x * x2, p, x);
  if (!(fabs(x) < 0.06)) {
    asm volatile("; rare: asin outside the series' range");
    r = asin(x);
  }
  return r;
}

// asin_small of two values at once (the two mirrors of phase B): both series step by step side by side in ONE basic block, so
// each coefficient is written to scalar registers once and read by two FMAs back to back.  Every chain does asin_small's
// operations in asin_small's order - the same bits; the library fall-backs stay per value, behind both series.
__device__ __forceinline__ void asin_small_pair(double xa, double xa2, double xb, double xb2, double& ra, double& rb) {
  double pa = 0.01396484375, pb = 0.01396484375;   // 143/10240
#define SART_STEP2(c) pa = HORNER(pa, xa2, c); pb = HORNER(pb, xb2, c)
  SART_STEP2(0.017352764423076924);                // 231/13312
  SART_STEP2(0.022372159090909092);                // 63/2816
  SART_STEP2(0.030381944444444444);                // 35/1152
  SART_STEP2(0.044642857142857144);                // 5/112
  SART_STEP2(0.075);                               // 3/40
  SART_STEP2(0.16666666666666666);                 // 1/6
#undef SART_STEP2
  ra = fma(xa * xa2, pa, xa);
  rb = fma(xb * xb2, pb, xb);
  if (!(fabs(xa) < 0.06)) {
    asm volatile("; rare: asin outside the series' range");
    ra = asin(xa);
  }
  if (!(fabs(xb) < 0.06)) {
    asm volatile("; rare: asin outside the series' range");
    rb = asin(xb);
  }
}

// atan for ray slopes (|x| < 0.05): alternating series to x^15; library outside.
__device__ __forceinline__ double atan_small(double x) {
  const double x2 = x * x;
  double p = -1.0 / 15.0;
  p = fma(p, x2, 1.0 / 13.0);
  p = fma(p, x2, -1.0 / 11.0);
  p = fma(p, x2, 1.0 / 9.0);
  p = fma(p, x2, -1.0 / 7.0);
  p = fma(p, x2, 1.0 / 5.0);
  p = fma(p, x2, -1.0 / 3.0);
  double r = fma(x * x2, p, x);
  if (!(fabs(x) < 0.05)) {
    asm volatile("; rare: atan outside the series' range");
    r = atan(x);
  }
  return r;
}

// cos on |x| <= 1 by its Taylor series to x^20 (error < 1e-19 there); library outside.
__device__ __forceinline__ double cos_small(double x) {
  const double x2 = x * x;
  double p = 4.110317623312165e-19;            //  1/20!
  p = fma(p, x2, -1.5619206968586225e-16);     // -1/18!
  p = fma(p, x2, 4.779477332387385e-14);       //  1/16!
  p = fma(p, x2, -1.1470745597729725e-11);     // -1/14!
  p = fma(p, x2, 2.08767569878681e-09);        //  1/12!
  p = fma(p, x2, -2.755731922398589e-07);      // -1/10!
  p = fma(p, x2, 2.48015873015873e-05);        //  1/8!
  p = fma(p, x2, -0.001388888888888889);       // -1/6!
  p = fma(p, x2, 0.041666666666666664);        //  1/4!
  p = fma(p, x2, -0.5);
  double r = fma(p, x2, 1.0);
  if (!(fabs(x) <= 1.0)) {
    asm volatile("; rare: cos outside the series' range");
    r = cos(x);
  }
  return r;
}

// cos(ya) for the yaw angle ya = -deg(atan(t)) of a ray with slope t, the degree value taken as radians - sic
// (:1598, :2101-2115): cos((180 / pi) atan t) as ONE even power series in t (composed at 60 digits, mpmath), valid for
// |t| < 0.006 (every ray from the Sun: |slope| < 4.7e-3), truncation error < 7e-18; the two-step evaluation outside.
__device__ __forceinline__ double cos_yaw_of_slope(double t) {
  const double x = t * t;
  double p = 2976939695167.2104;                  // t^12
  p = HORNER(p, x, -112889008417.68803);          // t^10
  p = HORNER(p, x, 2979383355.295581);            // t^8
  p = HORNER(p, x, -49735946.89381117);           // t^6
  p = HORNER(p, x, 450128.3326032301);            // t^4
  p = HORNER(p, x, -1641.403175005872);           // t^2 : -(180 / pi)^2 / 2
  double r = fma(p, x, 1.0);
  if (!(fabs(t) < 0.006)) {
    asm volatile("; rare: slope outside the composed series' range");
    r = cos_small(-atan_small(t) * 57.29577951308232);
  }
  return r;
}

// exp(x) for x <= 0 - the two exponentials of the gas stage, exp(-Gamma L / 2) and exp(-(mu_pipe d + mu_magnet L))
// (axionMassforMagnet.nim:75-113) - in 20 vector instructions instead of the library's ~40: n = rint(x log2 e),
// r = x - n ln 2 in two pieces (|r| <= 0.3466), Taylor series to r^13 (truncation 4e-18), one v_ldexp_f64.  <= 1.5 ulp
// (tests/test_gpu_math.py); x < -746 gives 0, like the library.
__device__ __forceinline__ double exp_neg(double x) {
  x = fmax(x, -746.0);
  const double n = __builtin_rint(x * 1.4426950408889634);
  double r = fma(n, -0.6931471805598903, x);         // ln 2, high part (low 11 bits zero: n * hi is exact)
  r = fma(n, -5.497923018708371e-14, r);             // ln 2, low part
  double p = 1.6059043836821613e-10;                 // 1/13!
  p = HORNER(p, r, 2.08767569878681e-09);            // 1/12!
  p = HORNER(p, r, 2.505210838544172e-08);           // 1/11!
  p = HORNER(p, r, 2.755731922398589e-07);           // 1/10!
  p = HORNER(p, r, 2.7557319223985893e-06);          // 1/9!
  p = HORNER(p, r, 2.48015873015873e-05);            // 1/8!
  p = HORNER(p, r, 0.0001984126984126984);           // 1/7!
  p = HORNER(p, r, 0.001388888888888889);            // 1/6!
  p = HORNER(p, r, 0.008333333333333333);            // 1/5!
  p = HORNER(p, r, 0.041666666666666664);            // 1/4!
  p = HORNER(p, r, 0.16666666666666666);             // 1/3!
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  return ldexp(p, (int)n);
}

// cos(y) for the phase q L of the gas-stage conversion probability (any finite y; thousands of radians far from the
// resonance): y / (2 pi) with 1 / (2 pi) in two pieces (the FMA keeps the product exact before the integer part is taken
// away, the second piece corrects it: the fraction of a turn is good to ~1e-16 for |y| < 1e15), then the table-based
// cosine of the sampling angles (sincos_turns: (cos, sin)(pi k / 64) from LDS + degree-3 polynomials).  Absolute error
// <= 2.5e-16 + 7e-16 |y| 2^-53 ... in practice <= 1.5 ulp(1); the library's Payne-Hanek path costs ~100 instructions.
__device__ __forceinline__ double cos_any(double y, const double* __restrict__ table, const SinCosCoef& K) {
  const double n = __builtin_rint(y * 0.15915494309189535);
  double f = fma(y, 0.15915494309189535, -n);        // 1 / (2 pi), high part
  f = fma(y, -9.839338337591243e-18, f);             // low part
  double sn, cs;
  sincos_turns<2>(fabs(f), table, K, &sn, &cs);      // cos is even; |f| <= 0.5 + 1e-16
  if (!(fabs(y) < 1e15)) {
    asm volatile("; rare: cos of a huge or non-finite phase");
    cs = cos(y);
  }
  return cs;
}

// Gas-stage conversion probability axionConversionProb2 (axionMassforMagnet.nim:75-98) of one ray for one axion mass:
//   P = (g B / 2)^2 / (q^2 + Gamma^2 / 4) (1 + exp(-Gamma L) - 2 exp(-Gamma L / 2) cos(q L)),   q = |m_gamma^2 - m_a^2| / (2 E)
// split into what depends on the ray alone (GasRay: built once per ray in phase B) and the mass (dm2_abs).  The histogram
// kernels apply it as the LAST factor of the weight, and the fused mass scan calls it once per mass on the same GasRay: every
// operation below is an explicit multiplication or FMA (nothing for the compiler to contract differently in different
// surroundings), so a scan's weight for mass k is bit for bit the weight of a single-mass launch with that mass.
struct GasRay {
  double inv_two_e;   // 1 / (2 E[eV])
  double g2q;         // Gamma^2 / 4
  double m2eh;        // -2 exp(-Gamma L / 2)
  double eh2p1;       // 1 + exp(-Gamma L)
  double Lnat;        // L in 1 / eV
};
// A value the compiler must keep in a vector register from here on (a polynomial's leading coefficient in front of a loop: with
// -disable-machine-licm nothing hoists the two v_mov_b32 that materialise an f64 constant out of a loop by itself).
__device__ __forceinline__ double in_vgpr(double x) {
  asm volatile("" : "+v"(x));
  return x;
}
// The leading coefficients of the two residual polynomials of the table-based cosine, in vector registers (GasCos::make() in
// front of the per-mass loop of the scan); the other five are scalar operands of the Horner steps.
struct GasCos {
  double s3, d3;
  static __device__ __forceinline__ GasCos make() { return GasCos{in_vgpr(SC(-0.5992645293207921)), in_vgpr(SC(-1.3352627688545895))}; }
};
// cos_any with every Horner step as v_fma_f64 v, v, v, s (fma_vvs): the same operations in the same order as cos_any /
// sincos_turns<2> - bit for bit the same cosine - but no coefficient is copied into a vector register per evaluation (LLVM
// otherwise selects v_fmac_f64 and moves each addend into its destination first: 12 v_mov_b32 per mass in the scan's loop, a
// quarter of its vector instructions).
__device__ __forceinline__ double cos_any_vvs(double y, const double* __restrict__ table, const GasCos& C) {
  const double n = __builtin_rint(y * 0.15915494309189535);
  double f = fma(y, 0.15915494309189535, -n);        // 1 / (2 pi), high part
  f = fma(y, -9.839338337591243e-18, f);             // low part
  const double u = fabs(f);                          // cos is even; |f| <= 0.5 + 1e-16
  const double kf = __builtin_rint(u * 128.0);
  const double r = fma(-1.0 / 64.0, kf, u * 2.0);
  const double2 t = reinterpret_cast<const double2*>(table)[(int)kf];
  const double x = r * r;
  const double sr = HORNER(HORNER(HORNER(C.s3, x, 2.5501640398773455), x, -5.16771278004997), x, 3.141592653589793) * r;
  const double cr = fma(HORNER(HORNER(C.d3, x, 4.0587121264167685), x, -4.934802200544679), x, 1.0);
  double cs = fma(-t.y, sr, t.x * cr);
  if (!(fabs(y) < 1e15)) {
    asm volatile("; rare: cos of a huge or non-finite phase");
    cs = cos(y);
  }
  return cs;
}
__device__ __forceinline__ double gas_conversion_prob(double dm2_abs, const GasRay& G, double term1, const double* __restrict__ table,
                                                      const GasCos& C) {
  const double q = dm2_abs * G.inv_two_e;
  const double term2 = frcp(fma(q, q, G.g2q));
  const double term3 = fma(G.m2eh, cos_any_vvs(q * G.Lnat, table, C), G.eh2p1);
  return (term1 * term2) * term3;
}

// The table pointers of a launch are read from the LDS copy of the parameter blob, where the compiler cannot see
// their address space and would emit flat_load (which counts on both vmcnt and lgkmcnt and so serialises against the
// LDS traffic of the same wave).  They always point to global memory: say so.
template <typename T>
using global_ptr = const __attribute__((address_space(1))) T*;
template <typename T>
__device__ __forceinline__ global_ptr<T> as_global(const T* p) {
  return (global_ptr<T>)p;
}

// An object in LDS seen through an address the compiler cannot fold: field accesses become ds_read with ONE base register
// and immediate offsets.  With the address known at compile time every access to a field beyond the 64 KB immediate range
// gets its own v_mov_b32 of the absolute address (one vector instruction per parameter read).
template <typename T>
__device__ __forceinline__ const T& lds_opaque(const T& obj) {
  typedef const __attribute__((address_space(3))) T* lds_ptr;
  uint32_t a = (uint32_t)(uintptr_t)(lds_ptr)&obj;
  asm volatile("" : "+v"(a));
  return *(const T*)(lds_ptr)(uintptr_t)a;
}

// lowerBound(a, key) with the answer known to lie in [lo, hi] (guide-table bracket):
// first index i with a[i] >= key  (std/algorithm.lowerBound semantics).
template <typename Ptr>
__device__ __forceinline__ int lower_bound_bracket(Ptr a, int lo, int hi, double key) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Roots of a z^2 + 2 hb z + c = 0 in the reference's naming:
//   root1 = (-hb - sqrt(hb^2 - a c)) / a,  root2 = (-hb + sqrt(hb^2 - a c)) / a     (:649-650)
// evaluated without cancellation (q-form); root1 is preferred, then root2, else miss (:651-656).
__device__ __forceinline__ bool pick_root(double a, double hb, double c, double zlo, double zhi, double& z, uint64_t& hit_m) {
  const double disc = fma(hb, hb, -a * c);
  const double sq = fsqrt_pos(disc);  // NaN for disc <= 0 -> every comparison below is false -> miss (disc == 0: tangent ray, measure zero)
  // q = -(hb + sign(hb) sq); the two roots are q / a and c / q.  With hb >= 0 (sign bit clear) q / a is the reference's
  // root1 and c / q its root2, with hb < 0 the other way round.
  const double q = -hb - copysign(sq, hb);
  const double raq = frcp(a * q);            // one reciprocal: 1/a = q raq, 1/q = a raq
  const double ra = q * q * raq, rb = c * a * raq;
  const bool a_lo = ra > zlo, a_hi = ra < zhi, b_lo = rb > zlo, b_hi = rb < zhi;
  const bool in_a = a_lo & a_hi, in_b = b_lo & b_hi;
  hit_m = (ballot64(a_lo) & ballot64(a_hi)) | (ballot64(b_lo) & ballot64(b_hi));   // the verdict as a lane mask (see phase_a_core)
  // root1 if it lies in the mirror's z range, else root2, else miss (:651-656): only when both roots are in range does
  // the order matter, and then root1 is q / a exactly when the sign bit of hb is clear
  const bool a_first = __double2hiint(hb) >= 0;
  z = (in_b & !(in_a & a_first)) ? rb : ra;
  return in_a | in_b;
}

// Reflection of the (un-normalised) direction w, |w|^2 = L, at a surface with (un-normalised)
// normal n, |n|^2 = N2:  the reference's v' = v cos 2a - (v x axis) sin 2a with a = asin|n.v|/|n|
// (:774-779) equals  v (1 - 2c^2 + 2c|c|) - 2|c| n^  with c = n^.v ; written for w = |w| v.
// Returns sin^2(a) = c^2 and, in sin_a, sin(a) = |c| (from the reciprocal square root the formula needs anyway: the
// reflectivity lookup wants the angle itself, and a separate square root of c^2 would cost seven more instructions).
__device__ __forceinline__ double reflect(double& wx, double& wy, double& wz, double L, double nx, double ny,
                                          double nz, double N2, double& sin_a) {
  const double dnw = fma(nx, wx, fma(ny, wy, nz * wz));
  const double y = frsq(N2 * L);             // 1 / (|n| |w|)
  const double rnl = y * y;                  // 1 / (N2 L): serves 1/N2 and 1/(N2 L)
  sin_a = fabs(dnw) * y;
  const double c2 = dnw * dnw * rnl;
  const double f = dnw * (L * rnl);
  const double ox = wx, oy = wy, oz = wz;
  wx = fma(-2.0 * f, nx, ox);                // mirror reflection (normal on the far side of the ray: n.w >= 0)
  wy = fma(-2.0 * f, ny, oy);
  wz = fma(-2.0 * f, nz, oz);
  if (dnw < 0.0) {                           // practically never taken (skipped when no lane needs it)
    // normal facing the ray: the reference's formula is then not a mirror reflection; keep it
    asm volatile("; rare: normal facing the ray");   // keeps LLVM from turning the block into always-executed selects
    const double k = 1.0 - 4.0 * c2;
    wx = fma(2.0 * f, nx, k * ox);
    wy = fma(2.0 * f, ny, k * oy);
    wz = fma(2.0 * f, nz, k * oz);
  }
  return c2;
}

// calcNormalVec (:731-759) z-component for an arbitrary point (general form with the square root; needed when the ray missed
// the mirror and the reference evaluates the normal at its input point: the rays that go on to the nickel test, an eighth of
// BabyIAXO's phase-B rays - some lane of nearly every pass).  rho / sqrt(w) = rho^2 / sqrt(rho^2 w): ONE reciprocal square root
// from the hardware seed (sart_math.h) instead of two IEEE square roots and a division (17 instead of ~90 vector instructions).
__device__ __forceinline__ double normal_z_general(const DevParams& P, const ShellDev& sh, int mirror, double x,
                                                   double y, double z) {
  const double rho2 = fma(x, x, y * y);
  if (!P.telescope_wolter) return (mirror == 1 ? sh.n1_tan : sh.n2_tan) * (rho2 * frsq(rho2));
  const double lz = P.l_mirror - z;
  if (mirror == 1) return sh.n1_r3t * (rho2 * frsq(rho2 * fma(sh.n1_e, lz, sh.n1_r3sq)));
  const double w = fma(sh.n2_e * lz, fma(lz, sh.n2_invF, 1.0), sh.n2_r3sq);
  return sh.n2_r3t * fma(2.0 * lz, sh.n2_invF, 1.0) * (rho2 * frsq(rho2 * w));
}

// ------------------------------------------------------------------------------------------------
// LDS-resident tables of one workgroup
// ------------------------------------------------------------------------------------------------
struct LdsTables {
  const double* sincos;      // (cos, sin)(pi k / 64), k = 0 .. 128
  const uint32_t* rcdf_hi;   // fluxRadiusCDF as the upper 32 of the 52 bits of floor(cdf 2^52), saturated (stage_tables)
  const double* rcdf_f64;    // the f64 table in device memory: decides the ties of the general form's 32-bit compare (one draw in ~1e9)
  const uint16_t* rguide;    // guide table in front of it
  const ShellDev* shells;
  const uint8_t* lut;        // radial look-up table of the shell selection
  // the radial verdict table (solar-source histogram kernels with HotA::radial_table set: `lut` then holds ITS cells) and the
  // shell selection's own cells in device memory, for the lanes of a marked cell
  const RadialLds* radial = nullptr;
  const DevTables* tabs = nullptr;   // (the LDS copy of the blob's pointers: shell_lut is fetched from it inside the rare block)
};

// State of a ray between phase A and phase B.
struct RayState {
  double X0, Y0;     // pointEntranceXRT (telescope frame, z = 0)
  double tsx, tsy;   // slopes dX/dz, dY/dz in the telescope frame
  double path_cb;    // path length inside the magnetic field
  double u5;         // uniform of the energy draw
  uint32_t u5_hi;    // its random word: u5 = u5_hi / 2^32 = u52(u5_hi, 0) when the uniforms come from the ray's Philox block
  double zcb;        // z of pointExitCB in the telescope frame (z0 of :2051)
  int r_idx;         // sampled solar radius index (row of diffFluxCDFs)
  int shell;         // hit layer
};

// The wave's sum of v in T's own arithmetic: double, long long, or unsigned long long where the values may have wrapped (modulo 2^64)
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// SART_ACCUM_FIXED64: rint(x * scale) as an integer, |x * scale| < 2^51, in one FMA and one 64-bit subtraction: adding
// 1.5 * 2^52 puts the sum into the binade whose unit in the last place is 1, so the FMA's single rounding (to nearest,
// ties to even) IS the rounding to an integer, and the integer sits in the low mantissa bits.
__device__ __forceinline__ long long to_fixed(double x, double scale) {
  constexpr double kMagic = 6755399441055744.0;   // 1.5 * 2^52
  return __double_as_longlong(fma(x, scale, kMagic)) - __double_as_longlong(kMagic);
}
__device__ __forceinline__ long long wave_sum_i64(long long v) { return wave_sum(v); }
// 8-byte slots of the accumulators hold doubles (SART_ACCUM_F64) or int64 bit patterns (SART_ACCUM_FIXED64)
__device__ __forceinline__ void atomic_add_slot_i64(double* slot, long long v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(slot), (unsigned long long)v);   // global_atomic_add_x2, no return
}

// Gather from an HBM-resident table: wave-uniform base (scalar registers) + 32-bit byte offset per lane.
typedef double d2 __attribute__((ext_vector_type(2)));   // native vector: loads as one 16-byte access
template <typename T>
__device__ __forceinline__ T gload(const void* base, uint32_t byte_off) {
  typedef const __attribute__((address_space(1))) char* gbytes;
  return *reinterpret_cast<const __attribute__((address_space(1))) T*>((gbytes)base + byte_off);
}

// Energy index drawn with u5 from the CDF row of the sampled radius (getRandomEnergyFromSolarModel, :444-471) =
// lowerBound(row, u5), in three steps that phase B spreads over its mirror arithmetic so that the gathers of the draw are in
// flight while the wave computes.  Two-level form (guide word -> four CDF candidates -> [energy row, reflectivities]):
//   begin       bucket of u5 (sart_device.h: kEnergyGuide*), gather of the guide word (entries k, k + 1 of the row)
//   candidates  bracket [lo, hi] from the guide word, gather of row[lo .. lo + 3] (rows are padded with 1.0)
//   finish      lo + #{candidates < u5}: the row is sorted and row[hi] >= u5, so candidates at or beyond hi never count;
//               only a lane whose four candidates are all < u5 with hi > lo + 4 goes on with a binary search
// Record form (word-exact draw with HotB::records_on; bucket record -> [energy row, reflectivities]):
//   begin       bucket of the word, gather of the bucket's 16-byte record (sart_device.h: kEnergyRecord*)
//   candidates  nothing
//   finish      the record's lo + #{its five thresholds below the word}; only a lane with a marked record and all five below goes
//               on, from lo + 5, with the guide's entry k + 1, four candidates and the binary search
typedef uint32_t u4v __attribute__((ext_vector_type(4)));   // native vector: loads as one 16-byte access
struct EnergyDraw {   // (two-level form | record form: the same registers, one form per launch)
  double u;
  uint32_t khi;        // upper 32 of the 52 bits of u 2^52 (word form: the word) | the same
  uint32_t row;        // element offset of the CDF row | the row's INDEX (the rare block forms both tables' offsets from it)
  uint32_t gword;      // guide entries k (low half) and k + 1 (high half) | unused
  uint32_t lo, hi;     // the guide's bracket | lo: the bucket k; hi: the word as the thresholds see it, (word - off) << 10
  u4v c;               // cdf_hi32 of row[lo .. lo + 3] | the bucket's record
};
// WORD (compile time): the uniform is a 32-bit random word over 2^32, u5 = word / 2^32 exactly (uniforms_of: every accumulating
// kernel).  Then  cdf < u5  <=>  cdf 2^32 < word  <=>  floor(cdf 2^32) < word  for every real cdf (word is an integer), and the
// saturated table entry 0xFFFFFFFF (cdf >= 1 - 2^-32) is never below a word: cdf_hi32 decides every candidate, there is no
// undecided case and no tie path; the bucket and the uniform / log split are shifts and compares of the word.  The general form
// (a uniform handed in from outside: the record kernel) makes no assumption about the bits of u5.
// The word form with bucket records (sart_device.h: kEnergyRecord*; HotB::records_on): ONE 16-byte gather in `begin` in place of the
// guide word and the candidates behind it, nothing in `candidates`, lo + #{thresholds of the record below the word} in `finish`.
// The switch is a flag in the kernel arguments, wave-uniform.  Each of the three places tests its own copy of the flag, taken
// through an empty asm: s_cmp_lg_u32 and a branch.  (One boolean shared by the three becomes a lane mask - s_cselect_b64, s_and_b64
// with exec, s_cbranch_vccnz at every use.)
__device__ __forceinline__ bool energy_records_on(const HotB& HB) {
  int32_t on = HB.records_on;
  asm volatile("" : "+s"(on));
  return on != 0;
}

// ---- configuration type of the histogram kernel body (sart_trace_histogram.inc), of phase A's second half and of phase B ----
// Every member answers one wave-uniform question that the hot path asks in every pass and whose answer is fixed for the whole
// launch.  RunTimeCfg answers by today's read of the kernel arguments or of the parameter block (every instantiation that
// existed before the folded form: the same code as without the type).  FoldedCfg answers with the constants of the reference's
// default configuration (sart_device.h: folded_form_applies is the host's side of the same list); the compare, the branch, the
// blocks it cuts and the constants re-materialised per block go away, the arithmetic stays.  Folded per group - stage A1, phase B,
// accumulation and loop - so that each group can be priced alone (experiment builds: -DSART_FOLD_A1=0 ...).
#ifndef SART_FOLD_A1
#define SART_FOLD_A1 1
#endif
#ifndef SART_FOLD_B
#define SART_FOLD_B 1
#endif
#ifndef SART_FOLD_ACC
#define SART_FOLD_ACC 1
#endif
// STRIPS: the strip loop of phase B is folded too (its trip count a constant: unrolled).  Vacuum only - in the gas-stage kernel the
// unrolled loop's eight bounds are live beside the absorption arithmetic and the kernel spills (128 VGPRs + 76 bytes of scratch per
// lane against 115 without), so its folded form keeps the loop.
template <bool A1, bool B, bool ACC, bool STRIPS>
struct HistCfg {
  // Which groups are folded.  At each place the body writes `CFG::kFoldX ? <the constant> : <the run-time read it always made>`: the
  // run-time arm stays the expression it was, so that the run-time form compiles to the code it had (a helper function around the
  // read, inlined, does not: the three tests of energy_records_on come out as one shared lane mask).
  static constexpr bool kFoldA1 = A1, kFoldB = B, kFoldAcc = ACC;
  static constexpr bool kFoldStrips = B && STRIPS;
  // the folded answers
  // stage A1: the radial verdict table is built; the optics are not the cone telescope; kFoldedSpokes spokes
  static constexpr int32_t kRadialTable = 1;
  static constexpr bool kIsLlnl = false;
  static constexpr int kSpokes = kFoldedSpokes;
  // phase B: the draw goes through the bucket records; Wolter optics; kFoldedHalfStrips strips (kFoldStrips); every flag of kFoldedFlags clear
  static constexpr bool kRecordsOn = true;
  static constexpr int kWolter = 1, kHalfStrips = kFoldedHalfStrips;
  // accumulation and loop: no spectra; stage A0 runs
  static constexpr int32_t kSpectra = 0;
  static constexpr bool kZones = true;
};
using RunTimeCfg = HistCfg<false, false, false, false>;
template <int GAS>
using FoldedCfg = HistCfg<SART_FOLD_A1 != 0, SART_FOLD_B != 0, SART_FOLD_ACC != 0, GAS == 0>;
static_assert(kFoldedFlags == (SART_CF_IGNORE_DET_WINDOW | SART_CF_IGNORE_GAS_ABS | SART_CF_IGNORE_REFLECTION | SART_CF_IGNORE_CONV_PROB |
                               SART_CF_XRAY_TEST), "the flags phase B tests");

template <bool WORD = false, class CFG = RunTimeCfg>
__device__ __forceinline__ void energy_draw_begin(const HotB& HB, int r_idx, double u5, uint32_t word, EnergyDraw& d, int r_idx_guide = -1) {
  if (r_idx_guide < 0) r_idx_guide = r_idx;   // (experiment builds pass another row for the guide gather: working-set sensitivity)
  d.u = u5;
  if (WORD) {
    d.khi = word;
  } else {
    // u5 = k 2^-52 exactly (u52: 52 random mantissa bits under the exponent of 1.0, minus 1.0): 1 + u5 carries k in its
    // mantissa, and its upper 32 bits are one funnel shift away.  (A uniform handed in from outside - the test entry - may
    // have bits below 2^-52: the sum then rounds k by at most 1/2, which energy_draw_finish allows for; the clamp keeps a
    // uniform within 2^-53 of 1 out of the next binade.)
    const double w = fmin(u5 + 1.0, 1.9999999999999998);
    d.khi = __builtin_amdgcn_alignbit((uint32_t)__double2hiint(w), (uint32_t)__double2loint(w), 20u);
  }
  static_assert((kEnergyGuideDiv & (kEnergyGuideDiv - 1)) == 0 && kEnergyGuideDiv >= 32, "the word form shifts by log2 of it");
  const double v = 1.0 - u5;
  // floor(u5 Div): of the word, its upper log2(Div) bits
  const uint32_t ku = WORD ? word >> (32 - __builtin_ctz((uint32_t)kEnergyGuideDiv)) : (uint32_t)(int)(u5 * (double)kEnergyGuideDiv);
  const uint32_t code = (uint32_t)__double2hiint(v) >> 14;                       // exponent and six mantissa bits of v
  const uint32_t kl = (uint32_t)kEnergyGuideUniform + min(kEnergyGuideCode0 - code, (uint32_t)kEnergyGuideLogMax);
  const bool uniform_bucket = WORD ? word < 0xF8000000u : v > 0.03125;           // u5 < 31/32: uniform buckets
  const uint32_t k = uniform_bucket ? ku : kl;
  if (WORD && (CFG::kFoldB ? CFG::kRecordsOn : energy_records_on(HB))) {
    // The bucket's record (sart_device.h: kEnergyRecord*) in ONE gather: lo and the first five entries of the bucket.  d.row keeps the
    // row and d.lo the bucket for the rare block of energy_draw_finish; d.hi is the word as the thresholds see it: one lower in the
    // log buckets, its low 22 bits moved to the top (a threshold sits in the upper 22 bits of its word, so the compare needs no
    // extraction).
    d.row = (uint32_t)r_idx;
    d.lo = k;
    d.hi = (word - (uint32_t)!uniform_bucket) << 10;
    d.c = gload<u4v>(HB.energy_records, (__umul24((uint32_t)r_idx_guide, (uint32_t)kEnergyGuideBuckets) + k) * 16u);
    return;
  }
  d.row = __umul24((uint32_t)r_idx, (uint32_t)HB.cdf_stride);                    // both < 2^24
  // two adjacent u16 as one (possibly unaligned) 32-bit load
  d.gword = gload<uint32_t>(HB.energy_guide, (__umul24((uint32_t)r_idx_guide, (uint32_t)kEnergyGuideEntries) + k) * 2u);
}
template <bool WORD = false, class CFG = RunTimeCfg>
__device__ __forceinline__ void energy_draw_candidates(const HotB& HB, EnergyDraw& d) {
  if (WORD && (CFG::kFoldB ? CFG::kRecordsOn : energy_records_on(HB))) return;   // nothing to issue: the record holds the candidates
  d.lo = d.gword & 0xFFFFu;
  d.hi = d.gword >> 16;
  // four consecutive u32 of a row whose stride is a multiple of four entries only by accident: the 16 bytes may straddle a
  // 16-byte boundary, global_load_dwordx4 needs 4-byte alignment only
  d.c = gload<u4v>(HB.cdf_hi32, (d.row + d.lo) * 4u);
}
template <bool WORD = false, class CFG = RunTimeCfg>
__device__ __forceinline__ int energy_draw_finish(const HotB& HB, const EnergyDraw& d) {
  const double u = d.u;
  if (WORD && (CFG::kFoldB ? CFG::kRecordsOn : energy_records_on(HB))) {
    // lowerBound = lo + #{thresholds of the record below the word}: four in the upper 22 bits of the record's words (whatever the
    // low ten bits hold, word < xs decides them: xs has zeros there), the fifth in the low bytes of words 1 - 3, which two byte
    // permutes put into the same form
    static_assert(kEnergyRecordK == 5 && kEnergyRecordEmpty == 0x3FFFFFu, "the layout energy_records_kernel packs");
    const uint32_t xs = d.hi;
    const uint32_t t4s = __builtin_amdgcn_perm(__builtin_amdgcn_perm(d.c.y, d.c.z, 0x04000c0cu), d.c.w, 0x0706000cu);
    const bool b4 = t4s < xs;
    uint32_t lo = ((d.c.x & 0x3FFu) | ((d.c.y & 0x100u) << 2)) + (uint32_t)(d.c.x < xs) + (uint32_t)(d.c.y < xs) + (uint32_t)(d.c.z < xs) +
                  (uint32_t)(d.c.w < xs) + (uint32_t)b4;
    // (the two conditions meet as lane masks on the scalar unit: as a per-lane bool the compiler builds the predicate from selects)
    if (__builtin_amdgcn_inverse_ballot_w64(ballot64(b4) & ballot64((d.c.w & 0x100u) != 0u))) {
      // more than five entries inside the bucket and all five below the word: the two-level draw from lo + 5 on
      asm volatile("; rare: energy bucket wider than its record");
      const uint32_t z = d.khi, row = __umul24(d.row, (uint32_t)HB.cdf_stride);
      const uint32_t hi = gload<uint16_t>(HB.energy_guide, (__umul24(d.row, (uint32_t)kEnergyGuideEntries) + d.lo + 1u) * 2u);
      const u4v c = gload<u4v>(HB.cdf_hi32, (row + lo) * 4u);
      const uint32_t lo5 = lo;
      lo += (uint32_t)(c.x < z) + (uint32_t)(c.y < z) + (uint32_t)(c.z < z) + (uint32_t)(c.w < z);
      if ((c.w < z) & (hi > lo5 + 4u)) {
        uint32_t h = hi;
        while (lo < h) {
          const uint32_t mid = (lo + h) >> 1;
          if (gload<double>(HB.diff_flux_cdfs, (row + mid) * 8u) < u) lo = mid + 1; else h = mid;
        }
      }
    }
    return (int)min(lo, (uint32_t)(HB.n_energies - 1));
  }
  if (WORD) {
    // lowerBound = lo + #{candidates < word}; only a bucket wider than four entries whose first four are all below goes on
    const uint32_t z = d.khi;
    uint32_t lo = d.lo + (uint32_t)(d.c.x < z) + (uint32_t)(d.c.y < z) + (uint32_t)(d.c.z < z) + (uint32_t)(d.c.w < z);
    if ((d.c.w < z) & (d.hi > d.lo + 4u)) {
      asm volatile("; rare: energy bucket wider than four entries");
      uint32_t hi = d.hi;
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (gload<double>(HB.diff_flux_cdfs, (d.row + mid) * 8u) < u) lo = mid + 1; else hi = mid;
      }
    }
    return (int)min(lo, (uint32_t)(HB.n_energies - 1));
  }
  // With T = floor(cdf 2^52) >> 20 (the table) and K = the upper 32 bits of u 2^52 rounded to an integer k':  T < K - 1 =>
  // floor(cdf 2^52) <= k' - 2^20 - 1 => cdf < u;  T > K => cdf 2^52 >= k' + 1 => cdf >= u (u 2^52 lies within 1/2 of k').
  // T in {K - 1, K}: undecided (2^-31 per candidate) - the f64 row decides, as it does in a wide bucket whose first four
  // entries are all below u.  (The 1.0 pads behind a row read 0xFFFFFFFF.)
  const uint32_t km1 = max(d.khi, 1u) - 1u;
  uint32_t lo = d.lo + (uint32_t)(d.c.x < km1) + (uint32_t)(d.c.y < km1) + (uint32_t)(d.c.z < km1) + (uint32_t)(d.c.w < km1);
  const bool tie = ((d.c.x - km1) < 2u) | ((d.c.y - km1) < 2u) | ((d.c.z - km1) < 2u) | ((d.c.w - km1) < 2u);
  if (((d.c.w < km1) & (d.hi > d.lo + 4u)) | tie) {
    asm volatile("; rare: energy bucket wider than four entries, or a tie in the upper 32 bits");
    if (tie) lo = d.lo;
    uint32_t hi = d.hi;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (gload<double>(HB.diff_flux_cdfs, (d.row + mid) * 8u) < u) lo = mid + 1; else hi = mid;
    }
  }
  return (int)min(lo, (uint32_t)(HB.n_energies - 1));
}
// the three steps back to back (record mode)
template <bool WORD = false>
__device__ __forceinline__ int sample_energy_index(const HotB& HB, int r_idx, double u5, uint32_t word = 0u) {
  EnergyDraw d;
  energy_draw_begin<WORD>(HB, r_idx, u5, word, d);
  energy_draw_candidates<WORD>(HB, d);
  return energy_draw_finish<WORD>(HB, d);
}

static_assert(sizeof(EnergyDev) == 8 * sizeof(double), "EnergyDev is loaded as eight f64");
__device__ __forceinline__ EnergyDev load_energy_row(const HotB& HB, int e_idx) {
  // field by field: the compiler merges neighbours and drops what a variant does not use (a wider load with a dead half
  // would have that half's registers reused while the gather is still in flight, which forces an early wait)
  const uint32_t off = (uint32_t)e_idx * 64u;
  return EnergyDev{gload<double>(HB.energy_tab, off), gload<double>(HB.energy_tab, off + 8u), gload<double>(HB.energy_tab, off + 16u),
                   gload<double>(HB.energy_tab, off + 24u), gload<double>(HB.energy_tab, off + 32u), gload<double>(HB.energy_tab, off + 40u),
                   gload<double>(HB.energy_tab, off + 48u), gload<double>(HB.energy_tab, off + 56u)};
}

// cos(n phi) from c = cos(phi) for the spoke test cos(n phi) >= cos(n w): Chebyshev T6 = T2(T3), or T16 by four doublings in
// scaled form, one FMA each: with u = c^2 - 1/2, v = u^2 - 1/8, w = v^2 - 1/128, z = w^2 - 1/32768 the doublings give
// T2 = 2u, T4 = 8v, T8 = 128w, T16 = 32768 z (powers of two: exact), so the function returns z and the host stores the
// threshold divided by 32768 (sart_api.hip: hot_of).
// The addends are scalar operands (HORNER: v_fma_f64 v, v, v, s): as literals LLVM copies each of them into the destination
// of a two-address v_fmac_f64 first, two v_mov_b32 per step (16 of the vector instructions of a phase-A pass).
__device__ __forceinline__ double spoke_measure(int n, double c) {
  if (n == 16) {
    const double u = HORNER(c, c, -0.5);
    const double v = HORNER(u, u, -0.125);
    const double w = HORNER(v, v, -0.0078125);
    return HORNER(w, w, -1.0 / 32768.0);
  }
  const double t3 = c * HORNER(4.0 * c, c, -3.0);
  return HORNER(2.0 * t3, t3, -1.0);
}

// spoke_measure of two cosines at once (entrance plane and spider plane): the two chains side by side, one pair of scalar
// moves per addend; the same operations in the same order per chain - the same bits as spoke_measure.
__device__ __forceinline__ void spoke_measure_pair(int n, double ca, double cb, double& ma, double& mb) {
  if (n == 16) {
    const double ua = HORNER(ca, ca, -0.5), ub = HORNER(cb, cb, -0.5);
    const double va = HORNER(ua, ua, -0.125), vb = HORNER(ub, ub, -0.125);
    const double wa = HORNER(va, va, -0.0078125), wb = HORNER(vb, vb, -0.0078125);
    ma = HORNER(wa, wa, -1.0 / 32768.0);
    mb = HORNER(wb, wb, -1.0 / 32768.0);
    return;
  }
  const double ta = ca * HORNER(4.0 * ca, ca, -3.0), tb = cb * HORNER(4.0 * cb, cb, -3.0);
  ma = HORNER(2.0 * ta, ta, -1.0);
  mb = HORNER(2.0 * tb, tb, -1.0);
}

// ------------------------------------------------------------------------------------------------
// phase A: sample -> bore -> pipes -> telescope frame -> opaque structures -> shell selection
// (:1746-1957).  Returns true if the ray goes on to the mirrors; `reached` = survived bore + pipes.
// st.r_idx / st.u5 are valid whenever the collimator cut (X-ray test source) was passed (`sampled`).
//
// Written in predicated form: every cut of the reference is an `ok &= ...` instead of an early return.
// A wave of 64 rays practically always has survivors up to the shell selection, so an early return
// saves no issue slots - it only costs exec-mask bookkeeping (SALU + SGPRs).  Lanes whose ray is dead
// keep computing on finite values; their results are discarded.
// ------------------------------------------------------------------------------------------------
//
// FAST = the configuration known at compile time to be: solar source (no X-ray test source), telescope
// not rotated, no hole loop in the optics.  The generic instantiation reads those switches at run time.
// ROT: telescope rotation known at compile time (0 / 1) or read at run time (-1).
// ZEXT: st.path_cb carries the z extent of the path in the magnetic field instead of its length (phase B of the vacuum,
// unrotated specialisation multiplies pathCB^2 by 1 + slope^2 itself and needs no square root here).
// The six uniforms of a ray in the reference's draw order: solar source u0, u1 -> angles of the solar point
// (:433-434), u2 -> radius CDF (:436), u3 -> disc radius (:418), u4 -> disc angle (:419), u5 -> energy CDF (:464).
struct Uniforms {
  double u0, u1, u2, u3, u4, u5;
  uint32_t u2_hi;   // floor(u2 2^32): the radius draw's guide bucket, and what it compares with the 32-bit copy of the CDF in LDS
  uint32_t u5_hi = 0u;   // uniforms_of: the word behind u5 (u5 = u52(u5_hi, 0)); unused for uniforms handed in from outside
};
// u2_hi of a uniform that does not come with its random words (the test entry of the record kernel)
__device__ __forceinline__ uint32_t upper32_of_uniform(double u) {
  return (uint32_t)(u * 4294967296.0);   // floor(u 2^32), exact for every u in [0, 1)
}
// phase A's verdicts as wave-wide lane masks (see phase_a_bore).  keep, cand (phase_a_telescope<.., RTAB = true> only): not below
// shell0_miss_radius / above mirror_miss_radius, for the lanes of `ok` (other lanes: any value)
struct LaneMasks { uint64_t ok, reached, keep, cand; };

// Phase A is written in two halves that meet where the magnet's pipes end and the telescope begins (:1868 | :1878): everything
// in the first half - sampling, bore, cold-bore exit, pipe cuts - is independent of the telescope's angles, everything in the
// second half depends on them.  The histogram and record kernels run them back to back (phase_a_core); the fused angular scan
// (trace_angular_scan_kernel) runs the first half once per ray and the second half once per ray and angle.
// What the first half hands to the second:
struct BoreRay {
  double x1, y1;     // the ray at the cold-bore exit (z = -Lp in the telescope's frame before its rotation)
  double x3, y3;     // ... and at the end of the second pipe (z = 0 there)
  double sx, sy;     // slopes dx/dz, dy/dz in the magnet frame
  bool ok;           // alive so far (= `reached`)
  uint64_t okm;      // the same as a lane mask
};
// The rotation of the telescope about (0, 0, lT/2) (:1888-1894) as hoist_setup() evaluates it (DevParams holds the same five
// values in the same order: phase_a_core takes them from there; the angular scan has one set per angle in its kernel arguments).
struct TelRot {
  double rx_c, rx_s, ry_c, ry_s, half_length_telescope;
};
static_assert(offsetof(DevParams, rx_s) == offsetof(DevParams, rx_c) + 8 && offsetof(DevParams, ry_c) == offsetof(DevParams, rx_c) + 16 &&
                  offsetof(DevParams, ry_s) == offsetof(DevParams, rx_c) + 24 && offsetof(DevParams, half_length_telescope) == offsetof(DevParams, rx_c) + 32,
              "TelRot mirrors these five fields of DevParams");
__device__ __forceinline__ const TelRot& tel_rot_of(const DevParams& P) { return *reinterpret_cast<const TelRot*>(&P.rx_c); }

// The radius draw of phase_a_bore: lowerBound(fluxRadiusCDF, u2) from the staged tables (u2_hi = floor(u2 2^32)).
template <bool WORD>
__device__ __forceinline__ int radius_draw(const LdsTables& L, uint32_t u2_hi, double u2) {
  // lowerBound(fluxRadiusCDF, u2) (:437).  K = floor(u2 2^32) picks the guide bucket (sart_device.h: 2048 buckets, and 1024
  // finer ones for u2 >= 31/32) whose two entries bracket the index.  The table sits in LDS as T = floor(cdf 2^32), saturated
  // (half the bytes of the f64 table: the other half is image tile; the 1.0 pads read 0xFFFFFFFF).
  // WORD: u2 = K / 2^32 exactly, so cdf < u2 <=> T < K: the count of the entries below K IS the lowerBound, nothing is undecided.
  // General form (u2 with bits below 2^-32), with T' = T + 1 saturated:  T' < K => cdf < u2;  T' > K + 1 => cdf > u2;
  // T' in {K, K + 1}: undecided, 2^-31 per entry looked at - the f64 table in device memory decides.
  const uint32_t khi = u2_hi;
  const uint32_t kb = khi >> 21, kt = (khi >> 17) - ((kRadiusGuideTopStart >> 17) - (uint32_t)(kRadiusGuide + 1));
  const uint32_t k = khi >= kRadiusGuideTopStart ? kt : kb;
  const int lo0 = (int)L.rguide[k];
  const int hi0 = (int)L.rguide[k + 1];
  auto entry = [&](int i) {   // T (WORD) or T'
    const uint32_t t = L.rcdf_hi[i];
    return WORD ? t : t + (uint32_t)(t != 0xFFFFFFFFu);
  };
  // four consecutive candidates in ONE round trip to LDS: the table is sorted and rcdf[hi] >= u2, so entries at or beyond hi
  // never count (the stage pads the table with four entries of 1.0)
  const uint32_t c0 = entry(lo0), c1 = entry(lo0 + 1), c2 = entry(lo0 + 2), c3 = entry(lo0 + 3);
  int lo = lo0 + (int)(c0 < khi) + (int)(c1 < khi) + (int)(c2 < khi) + (int)(c3 < khi);
  // undecided: an entry in {K, K + 1}, i.e. the smallest of the four differences (unsigned: entries below K wrap to huge) < 2
  bool tie = WORD ? false : min(min(c0 - khi, c1 - khi), min(c2 - khi, c3 - khi)) < 2u;
  if ((c3 < khi) & (hi0 > lo0 + 4)) {
    asm volatile("; rare: radius bucket wider than four entries");
    int hi = hi0;
    while (lo < hi) {   // first entry that is not (certainly) below u2
      const int mid = (lo + hi) >> 1;
      if (entry(mid) < khi) lo = mid + 1; else hi = mid;
    }
    if (!WORD) tie = (entry(lo) - khi) < 2u;   // that entry is undecided (everything behind it is >= it; the four in front were certain)
  }
  if (!WORD && tie) {
    asm volatile("; rare: a tie in the upper 32 bits of the radius draw");
    lo = lower_bound_bracket(as_global(L.rcdf_f64), lo0, hi0, u2);
  }
  return lo;
}

// ---- first half: sample -> bore -> cold-bore exit -> pipes (:1746-1868) ----
// WORD: the uniforms are the ray's random words over 2^32 (uniforms_of) - the word-exact CDF draws (energy_draw_begin).
template <bool FAST, bool ZEXT, bool NOWALL = false, bool WORD = false>
__device__ __forceinline__ void phase_a_bore(const HotA& H, const DevParams& P, const LdsTables& L, const Uniforms& U, RayState& st,
                                             bool& sampled, bool& reached, BoreRay& br, LaneMasks& M, const SinCosCoef* held = nullptr) {
  const bool cfg_test = FAST ? false : (H.test_active != 0);
  const double u0 = U.u0, u1 = U.u1, u2 = U.u2, u3 = U.u3, u4 = U.u4;
  st.u5 = U.u5;
  st.u5_hi = U.u5_hi;
  st.r_idx = 0;

  bool ok = true;
  double ex, ey;            // point on the magnetic-field exit plane z = lengthB
  double sx, sy;            // ray slopes dx/dz, dy/dz in the magnet frame
  if (!cfg_test) {
    // getRandomPointFromSolarModel (:425-442): theta1 = 360 u0 deg, theta2 = 180 u1 deg (uniform in theta)
    double s1, c1, s2, c2;
    // one set of constants for the three evaluations: scalar, written here, or the caller's copy in vector registers (`held`)
    const SinCosCoef K = held ? *held : sincos_coef();
    sincos_turns<2>(u0, L.sincos, K, &s1, &c1);
    sincos_turns<1>(u1, L.sincos, K, &s2, &c2);
    st.r_idx = radius_draw<WORD>(L, U.u2_hi, u2);
    const double r = (0.0015 + (double)st.r_idx * 0.0005) * H.sun_radius;
    const double ox = c1 * s2 * r, oy = s1 * s2 * r, oz = c2 * r - H.sun_distance;
    // getRandomPointOnDisk (:412-422)
    double sp, cp;
    sincos_turns<2>(u4, L.sincos, K, &sp, &cp);
    // + 1e-300: exact no-op unless u3 == 0 (one ray in 2^44: its point lands 1e-150 R from the axis instead of on it); saves
    // the zero / negative special-casing of fsqrt() (two compares, four selects) in every pass
    const double rr = H.radius_cb * fsqrt_pos(u3 + 1e-300);
    ex = cp * rr;
    ey = sp * rr;
    const double inv_dz = frcp(H.length_b - oz);
    sx = (ex - ox) * inv_dz;
    sy = (ey - oy) * inv_dz;
  } else {
    // X-ray test source (:1765-1806)
    double sp, cp;
    const SinCosCoef K = sincos_coef();
    sincos_turns<2>(u1, L.sincos, K, &sp, &cp);
    const double rr = P.test_radius * fsqrt(u0);
    const double ox = cp * rr + P.test_x, oy = sp * rr + P.test_y, oz = P.test_z;
    if (P.test_parallel) {
      ex = ox + (u2 * 0.5) - 0.25;
      ey = oy + (u3 * 0.5) - 0.25;
    } else {
      double sq, cq;
      sincos_turns<2>(u3, L.sincos, K, &sq, &cq);
      const double r2 = H.radius_cb * fsqrt(u2);
      ex = cq * r2;
      ey = sq * r2;
    }
    const double inv_dz = frcp(H.length_b - oz);
    sx = (ex - ox) * inv_dz;
    sy = (ey - oy) * inv_dz;
    // collimator (:1800): lineIntersectsCircle(origin, exit point, collimator, source radius)
    const double dzc = P.test_collimator_z - H.length_b;
    const double cx = fma(dzc, sx, ex) - P.test_x, cy = fma(dzc, sy, ey) - P.test_y;
    ok = fma(cx, cx, cy * cy) < P.test_radius_sq;
  }
  sampled = ok;
  // The same verdicts as lane masks, combined on the scalar unit from the ballots of the single compares (the ballot of a
  // direct compare is the compare's own result; a ballot of `a & b & c` costs a select and a second compare): what the
  // histogram kernel counts and compacts with.  The bools stay for the divergent regions and for the record kernel.
  uint64_t okm = cfg_test ? ballot64(ok) : ~0ull;

  // ---- bore (:1813-1848) ----
  const double A2 = fma(sx, sx, sy * sy);     // slope^2
  const double norm = ZEXT ? 1.0 : fsqrt_pos(1.0 + A2);   // ZEXT: phase B applies the factor (1 + A2) to pathCB^2 itself
  // entrance plane z = 0
  double path_cb = H.length_b * norm;          // |exit point - entrance-plane point| (:1836-1843); FAST: its z extent
  // NOWALL (constant-path variant): the host has proved that no ray that passes the three cuts below entered through the bore
  // wall (sart_api.hip: path_is_constant), so a wall entry changes neither `ok` after those cuts nor `reached`, and nobody
  // reads the path: the entrance-plane test and the wall branch are not compiled.
  bool hits_entrance = true;
  if (!NOWALL) {
    const double x0 = fma(-H.length_b, sx, ex), y0 = fma(-H.length_b, sy, ey);
    hits_entrance = fma(x0, x0, y0 * y0) < H.radius_cb_sq;
  }
  if (!NOWALL && (ok & !hits_entrance)) {      // divergent, skipped when no lane needs it: the ray entered through the bore wall
    // lineIntersectsCylinderOnce (:591-604): intersections of the line with the bore wall,
    // t = z - lengthB:  A2 t^2 + 2 Dm t + (Qm - R^2) = 0.  inter1 = larger z, inter2 = smaller z.
    const double Dm = fma(ex, sx, ey * sy);
    const double c = fma(ex, ex, ey * ey) - H.radius_cb_sq;
    const double sq = fsqrt(fma(Dm, Dm, -A2 * c));
    const double q = (Dm >= 0.0) ? (-Dm - sq) : (-Dm + sq);
    const double qa = q * frcp(A2), cq = c * frcp(q);
    const double t_lo = (Dm >= 0.0) ? qa : cq, t_hi = (Dm >= 0.0) ? cq : qa;
    const double z_hi = H.length_b + t_hi, z_lo = H.length_b + t_lo;
    const bool v1 = (z_hi > 0.0) && (z_hi < H.length_coldbore);
    const bool v2 = (z_lo > 0.0) && (z_lo < H.length_coldbore);
    const double t = v1 ? t_hi : t_lo;         // :616
    ok = (v1 != v2);                           // exactly one valid intersection (:598-600, :1825)
    path_cb = fabs(t) * norm;
  }
  if (!NOWALL) okm = ballot64(ok);             // `ok` may come out of the divergent region above
  st.path_cb = path_cb;
  // exit of the cold bore (:1846), pipe CB -> VT3 (:1856), VT3 -> XRT (:1866; same radius — sic)
  const double x1 = fma(H.dz1, sx, ex), y1 = fma(H.dz1, sy, ey);
  const double x2 = fma(H.dz2, sx, ex), y2 = fma(H.dz2, sy, ey);
  const double x3 = fma(H.dz3, sx, ex), y3 = fma(H.dz3, sy, ey);
  // bitwise on purpose: `&&` keeps the short-circuit as three nested divergent regions (exec-mask bookkeeping around eight
  // f64 operations that nearly every lane needs anyway)
  const bool in1 = fma(x1, x1, y1 * y1) < H.radius_cb_sq, in2 = fma(x2, x2, y2 * y2) < H.pipe1_radius_sq,
             in3 = fma(x3, x3, y3 * y3) < H.pipe1_radius_sq;
  ok = ok & in1 & in2 & in3;
  okm &= ballot64(in1) & ballot64(in2) & ballot64(in3);
  reached = ok;
  M.reached = okm;
  br.x1 = x1; br.y1 = y1; br.x3 = x3; br.y3 = y3; br.sx = sx; br.sy = sy;
  br.ok = ok;
  br.okm = okm;
}

// ---- second half: telescope frame -> opaque structures -> shell selection (:1878-1957) ----
// `R`: the telescope's rotation; `shell0`-style shortcuts stay with the caller.  Returns true if the ray goes on to the mirrors.
// `r3sq` (optional): n1_r3sq of the selected shell - the squared radius of its paraboloid at z = l_mirror - for the caller's
// mirror-miss shortcut.
//
// ---- the verdicts that the radial distance alone decides, as one byte: code << 6 | shell (sart_device.h: RadialLds) ----
// By the compares: phase_a_telescope's own expressions for the inner disc, the XMM ring, the last shell, the shell selection and
// the glass front, and the two sure-miss radii of trace_histogram_kernel's stage A1 (`cand_on`: the mirror-miss shortcut is
// compiled in and the telescope is not the cone one).  `lut`: the shell selection's cells in device memory.  This is what the host
// evaluates around every breakpoint to fill the table (sart_api.hip: radial_verdict_of), and what the lanes of a marked cell run.
__device__ __forceinline__ uint32_t radial_verdict_compares(const HotA& H, const DevParams& P, const ShellDev* shells, const uint8_t* lut,
                                                            bool cand_on, double radial) {
  bool ok = true;
  if (H.telescope_kind != SART_TK_LLNL) {
    const bool inner = (H.telescope_kind == SART_TK_XMM) ? (radial <= H.inner_radius) : (radial < H.inner_radius);
    const bool ring = (H.telescope_kind == SART_TK_XMM) & (radial < H.ring_hi) & (radial > H.ring_lo);
    ok = !(inner | ring);
  }
  ok = ok & !(radial > H.r1_last);
  const int nS = H.n_shells;
  const int j0 = (int)as_global(lut)[max(min((int)(radial * H.lut_inv_step), H.lut_n - 1), 0)];
  const int jc = min(j0, nS - 1), jb = max(jc - 1, 0);
  const double c_r1 = shells[jc].r1, c_ro = shells[jc].r1_outer;
  const double b_r1 = shells[jb].r1, b_ro = shells[jb].r1_outer;
  const bool step = (j0 < nS) & !(c_r1 > radial);
  const int j = j0 + (step ? 1 : 0);
  ok = ok & (j < nS);
  const double g_r1 = step ? c_r1 : b_r1, g_ro = step ? c_ro : b_ro;
  ok = ok & !((j > 0) & (radial > g_r1) & (radial < g_ro));
  const uint32_t shell = (uint32_t)min(j, nS - 1);
  const uint32_t code = !ok ? 0u : (radial < P.shell0_miss_radius) ? 1u : (cand_on & (radial > (double)P.mirror_miss_radius)) ? 3u : 2u;
  return code << 6 | shell;
}
// By the table: the cell's byte, the breakpoint and its three verdicts read together, two compares, an extract.  A breakpoint in a
// lower cell than the ray's is below the ray's radial distance, one in a higher cell above it (a product by a positive constant and
// a truncation are monotone): only a breakpoint in the ray's own cell needs the compare, and the host allows one per cell.  (A
// marked lane reads entry kRadialMarked behind the table - cells of the image tile, still LDS of this workgroup - and drops it.)
__device__ __forceinline__ uint32_t radial_verdict_table(const HotA& H, const DevParams& P, const LdsTables& L, bool cand_on, double radial) {
  const uint32_t k = L.lut[max(min((int)(radial * H.lut_inv_step), H.lut_n - 1), 0)];
  const double b = L.radial->b[k];
  const uint32_t w = L.radial->w[k];
  uint32_t sh = (radial >= b) ? 8u : 0u;
  sh = (radial > b) ? 16u : sh;
  uint32_t v = (w >> sh) & 0xFFu;
  if (k == (uint32_t)kRadialMarked) {   // divergent, rare: several breakpoints in one cell; cell 0 (an unordered radial distance lands there)
    asm volatile("; rare: marked cell of the radial verdict table");
    v = radial_verdict_compares(H, P, L.shells, L.tabs->shell_lut, cand_on, radial);
  }
  return v;
}

// RTAB (solar-source histogram kernels): with HotA::radial_table set the radial verdicts come from the table; M.keep and M.cand are
// filled either way, and `r3sq` is not (the caller reads it for the selected shell where it needs it).
template <bool FAST, int ROT, bool RTAB = false, class CFG = RunTimeCfg>
__device__ __forceinline__ bool phase_a_telescope(const HotA& H, const DevParams& P, const TelRot& R, const LdsTables& L, const BoreRay& br,
                                                  RayState& st, double& radial_out, LaneMasks& M, double* r3sq = nullptr) {
  static_assert(!RTAB || (FAST && ROT >= 0), "the table serves the solar-source specialisations (no hole loop)");
  const bool cfg_rotated = (ROT < 0) ? (H.rotated != 0) : (ROT != 0);
  const bool cfg_holes = FAST ? false : (H.telescope_kind == SART_TK_XMM && H.inner_blocks < 0);
  const double x1 = br.x1, y1 = br.y1, x3 = br.x3, y3 = br.y3, sx = br.sx, sy = br.sy;
  bool ok = br.ok;
  uint64_t okm = br.okm;

  // ---- telescope frame (:1878-1899) ----
  // pointExitCB' (z = -Lp before rotation) and pointExitPipeVT3XRT' (z = 0 before rotation)
  const double Lp = H.dz3 - H.dz1;
  double X0, Y0, tsx, tsy, zcb;
  if (!cfg_rotated) {
    X0 = x3 - H.entrance_x;
    Y0 = y3 - H.entrance_y;
    tsx = sx;
    tsy = sy;
    zcb = -Lp;
  } else {
    // rotateInY(rotateInX(p, turnedX, lT/2), turnedY, lT/2) applied to both points (:1888-1894)
    auto rot = [&](double px, double py, double pz, double& qx, double& qy, double& qz) {
      const double zz = pz - R.half_length_telescope;
      const double ax = fma(px, R.rx_c, zz * R.rx_s);
      const double az = fma(zz, R.rx_c, -px * R.rx_s);   // rotateInX adds lT/2 back, rotateInY removes it again
      qx = ax;
      qy = fma(py, R.ry_c, -az * R.ry_s);
      qz = fma(az, R.ry_c, py * R.ry_s) + R.half_length_telescope;
    };
    double ax, ay, az, bx, by, bz;
    rot(x1, y1, -Lp, ax, ay, az);
    rot(x3, y3, 0.0, bx, by, bz);
    ax -= H.entrance_x; ay -= H.entrance_y;
    bx -= H.entrance_x; by -= H.entrance_y;
    const double inv = frcp(bz - az);
    tsx = (bx - ax) * inv;
    tsy = (by - ay) * inv;
    X0 = fma(-az, tsx, ax);     // pointEntranceXRT: z = 0 (:1897-1898)
    Y0 = fma(-az, tsy, ay);
    zcb = az;
  }
  st.X0 = X0; st.Y0 = Y0; st.tsx = tsx; st.tsy = tsy; st.zcb = zcb;
  const double Q0 = fma(X0, X0, Y0 * Y0);
  const double inv_radial = frsq(Q0);
  const double radial = Q0 * inv_radial;       // radialDist (:1905)

  if constexpr (RTAB) {
    if (CFG::kFoldA1 ? CFG::kRadialTable : H.radial_table) {   // wave-uniform
      // the spider's spokes as below; everything else the opaque structures and the shell selection decide is one verdict byte
      if (CFG::kFoldA1 ? !CFG::kIsLlnl : H.telescope_kind != SART_TK_LLNL) {
        const double c_ent = X0 * inv_radial;
        const double xs = fma(H.spider_z, tsx, X0), ys = fma(H.spider_z, tsy, Y0);
        const double c_sp = xs * frsq(fma(xs, xs, ys * ys));
        double meas_a, meas_b;
        spoke_measure_pair(CFG::kFoldA1 ? CFG::kSpokes : H.spoke_n, c_ent, c_sp, meas_a, meas_b);
        const bool spoke_a = meas_a >= H.spoke_cos_thr, spoke_b = meas_b >= H.spoke_cos_thr;
        ok = ok & !(spoke_a | spoke_b);
        okm &= ~(ballot64(spoke_a) | ballot64(spoke_b));
      }
      const uint32_t v = radial_verdict_table(H, P, L, ROT == 0 && (CFG::kFoldA1 ? !CFG::kIsLlnl : H.telescope_kind != SART_TK_LLNL), radial);
      M.ok = okm & ballot64(v > 63u);
      M.keep = ballot64(v > 127u);
      M.cand = ballot64(v > 191u);
      st.shell = (int)(v & 63u);
      radial_out = radial;
      return ok & (v > 63u);
    }
  }

  // ---- opaque structures (:1635-1704) ----
  if (H.telescope_kind != SART_TK_LLNL) {      // LLNL: the graphite block never blocks (:1646)
    const bool inner_le = radial <= H.inner_radius, inner_lt = radial < H.inner_radius;
    const bool inner = (H.telescope_kind == SART_TK_XMM) ? inner_le : inner_lt;
    // htNone: the hole test is always false => inner disc blocked (:1683-1688, :527); Abrixas :1653;
    // XMM ring :1691; spider spokes tested on phi = acos(x / r) at the entrance plane and at
    // z = spider_z (:1695-1701): every 360/n degrees, |phi - k 360/n| <= w  <=>  cos(n phi) >= cos(n w)
    const bool ring_a = radial < H.ring_hi, ring_b = radial > H.ring_lo;
    const bool ring = (H.telescope_kind == SART_TK_XMM) & ring_a & ring_b;
    const double c_ent = X0 * inv_radial;
    const double xs = fma(H.spider_z, tsx, X0), ys = fma(H.spider_z, tsy, Y0);
    const double c_sp = xs * frsq(fma(xs, xs, ys * ys));
    // (bitwise: the second test is needed by every lane the first one does not block - no divergent region around it)
    double meas_a, meas_b;
    spoke_measure_pair(H.spoke_n, c_ent, c_sp, meas_a, meas_b);
    const bool spoke_a = meas_a >= H.spoke_cos_thr, spoke_b = meas_b >= H.spoke_cos_thr;
    const bool spoke = spoke_a | spoke_b;
    bool blocked = inner | ring | spoke;
    const bool xmm = H.telescope_kind == SART_TK_XMM;   // wave-uniform
    uint64_t blocked_m = (xmm ? ballot64(inner_le) : ballot64(inner_lt)) | (xmm ? (ballot64(ring_a) & ballot64(ring_b)) : 0ull) |
                         ballot64(spoke_a) | ballot64(spoke_b);
    if (cfg_holes) {
      // hole loop (:1675-1688) with lineIntersectsObject (:494-527) on the entrance plane; replaces the
      // verdict for rays inside the inner disc
      const int nH = P.number_of_holes;
      const int lim = nH - (int)ceil((double)nH / 2.0);
      bool res = false, done = false;
      for (int l = -lim; l <= lim; ++l) {
        double hx = 0.0, hy = 0.0;
        if (l != 0) {
          if ((abs(l) & 1) == 0) hy += 2.0 * (double)l * P.hole_in_optics;
          else hx += 2.0 * ((double)l + ((double)l / (double)abs(l))) * P.hole_in_optics;
        }
        const double ix = X0 - hx, iy = Y0 - hy, rad = P.hole_in_optics;
        const double tx = ix / sqrt(2.0) - iy / sqrt(2.0), ty = ix / sqrt(2.0) + iy / sqrt(2.0);
        const double axx = fabs(ix), ayy = fabs(iy), atx = fabs(tx), aty = fabs(ty);
        bool through = false;
        switch (P.hole_type) {
          case SART_HT_CIRCLE: through = sqrt(fma(ix, ix, iy * iy)) < rad; break;
          case SART_HT_CROSS:
            through = (axx < rad && ayy < rad * 16.0) || (ayy < rad && axx < rad * 16.0); break;
          case SART_HT_STAR:
            through = (axx < rad && ayy < rad * 16.0) || (ayy < rad && axx < rad * 16.0) ||
                      (atx < rad && aty < rad * 16.0) || (aty < rad && atx < rad * 16.0); break;
          case SART_HT_SQUARE: through = axx < rad && ayy < rad; break;
          case SART_HT_DIAMOND: through = atx < rad && aty < rad; break;
          default: through = false;
        }
        if (!done) { res = !through; done = through; }   // `break` at the first hole the ray passes through
      }
      if (inner) blocked = res;
      blocked_m = ballot64(blocked);
    }
    ok = ok & !blocked;
    okm &= ~blocked_m;
  }

  // ---- shell selection (:1932-1957) ----
  const bool beyond = radial > H.r1_last;
  ok = ok & !beyond;
  okm &= ~ballot64(beyond);
  // R1 ascending: the nearest shell above is the first j with R1[j] > radial; the look-up cell (narrower
  // than any shell spacing) gives it up to one step
  const int nS = H.n_shells;
  const int j0 = (int)L.lut[max(min((int)(radial * H.lut_inv_step), H.lut_n - 1), 0)];
  // the radii of the cell's shell and of the one below it, read together (one round trip to LDS instead of two dependent ones)
  const int jc = min(j0, nS - 1), jb = max(jc - 1, 0);
  const double c_r1 = L.shells[jc].r1, c_ro = L.shells[jc].r1_outer;
  const double b_r1 = L.shells[jb].r1, b_ro = L.shells[jb].r1_outer;
  const bool step = (j0 < nS) & !(c_r1 > radial);
  const int j = j0 + (step ? 1 : 0);
  const bool has_shell = j < nS;
  ok = ok & has_shell;   // radial == R1[last] exactly (measure zero; the reference then uses a zero shell)
  okm &= ballot64(has_shell);
  // glass front (:1942-1944): only the shell just below the selected one can contain radial (thickness < spacing, checked on
  // the host): the cell's shell after a step, the one below it otherwise
  const double g_r1 = step ? c_r1 : b_r1, g_ro = step ? c_ro : b_ro;
  const bool gf_a = j > 0, gf_b = radial > g_r1, gf_c = radial < g_ro;
  ok = ok & !(gf_a & gf_b & gf_c);
  // (mask form: both candidates compared, the choice between them made on the masks - four compares instead of four selects
  // and two compares)
  const uint64_t step_m = ballot64(j0 < nS) & ~ballot64(c_r1 > radial);
  const uint64_t in_c = ballot64(radial > c_r1) & ballot64(radial < c_ro), in_b = ballot64(radial > b_r1) & ballot64(radial < b_ro);
  okm &= ~(ballot64(gf_a) & ((step_m & in_c) | (~step_m & in_b)));
  M.ok = okm;
  st.shell = min(j, nS - 1);
  radial_out = radial;
  if (r3sq) {
    // read beside c_r1 / c_ro for the cell's shell and the one above it (the selected shell is one of the two): no LDS round trip
    // behind the selection.  (jc + 1 == nS only for a ray without a shell; the record behind the last one is still LDS of the table
    // block, and `ok` is false for that ray.)
    const double c_r3sq = L.shells[jc].n1_r3sq, u_r3sq = L.shells[jc + 1].n1_r3sq;
    *r3sq = step ? u_r3sq : c_r3sq;
  }
  if constexpr (RTAB) {   // the caller's two compares (no table for this setup)
    M.keep = ~ballot64(radial < P.shell0_miss_radius);
    M.cand = (ROT != 0) ? 0ull : ballot64(radial > (double)P.mirror_miss_radius);
  }
  return ok;
}

// Both halves back to back (histogram and record kernels).
template <bool FAST, int ROT, bool ZEXT, bool NOWALL = false, bool WORD = false, bool RTAB = false, class CFG = RunTimeCfg>
__device__ __forceinline__ bool phase_a_core(const HotA& H, const DevParams& P, const LdsTables& L, const Uniforms& U, RayState& st,
                                             bool& sampled, bool& reached, double& radial_out, LaneMasks& M, const SinCosCoef* held = nullptr,
                                             double* r3sq = nullptr) {
  static_assert(!ZEXT || (FAST && ROT == 0), "the z-extent form needs the magnet-frame slopes in phase B");
  static_assert(!NOWALL || ZEXT, "the constant-path form is a specialisation of the vacuum, unrotated one");
  BoreRay br;
  phase_a_bore<FAST, ZEXT, NOWALL, WORD>(H, P, L, U, st, sampled, reached, br, M, held);
  return phase_a_telescope<FAST, ROT, RTAB, CFG>(H, P, tel_rot_of(P), L, br, st, radial_out, M, r3sq);
}

// Phase A of the ray with global id `ray_id`: its six uniforms from ONE Philox counter block (x, y, z, w) + its word s of the
// shared stream (sart_oracle_uniforms) - 160 random bits, none used twice:
//   u2 (radius CDF draw)  = x / 2^32            u5 (energy CDF draw) = z / 2^32          u3 (disc radius) = s / 2^32
//   u0 (solar point, theta1) = (y >> 11) / 2^21    u1 (theta2) = (w >> 11) / 2^21
//   u4 (disc angle) = ((y & 0x7FF) << 11 | (w & 0x7FF)) / 2^22
// 2^-21 of a turn is 3e-6 rad of position on a source 4.6e-3 rad wide seen from the magnet; 2^-22 of a turn on the bore-exit disc
// is under a micrometre of arc; the CDF draws resolve 2^-32 where the tables' entries are 5e-4 (radius) and ~7e-4 (energy) apart.
// u3_hi = word ray_id of the shared stream.
__device__ __forceinline__ Uniforms uniforms_of(uint32_t seed_lo, uint32_t seed_hi, uint64_t ray_id, uint32_t u3_hi) {
  const uint32_t id_lo = (uint32_t)ray_id, id_hi = (uint32_t)(ray_id >> 32);
  const U4 b0 = philox4x32(id_lo, id_hi, 0u, 0u, seed_lo, seed_hi);
  Uniforms U;
  U.u2 = u52(b0.x, 0u);
  U.u2_hi = b0.x;   // floor(u2 2^32) is the word itself
  U.u5 = u52(b0.z, 0u);
  U.u5_hi = b0.z;
  U.u0 = u52(b0.y & 0xFFFFF800u, 0u);
  U.u1 = u52(b0.w & 0xFFFFF800u, 0u);
  U.u4 = u52((b0.y << 21) | ((b0.w & 0x7FFu) << 10), 0u);
  U.u3 = u52(u3_hi, 0u);
  return U;
}
// (WORD = false: the record kernel, which keeps the general draws for both sources of its uniforms)
template <bool FAST, int ROT, bool ZEXT, bool NOWALL = false, bool WORD = true, bool RTAB = false, class CFG = RunTimeCfg>
__device__ __forceinline__ bool phase_a(const HotA& H, const DevParams& P, const LdsTables& L, uint32_t seed_lo,
                                        uint32_t seed_hi, uint64_t ray_id, uint32_t u3_hi, RayState& st, bool& sampled,
                                        bool& reached, double& radial, LaneMasks& M, const SinCosCoef* held = nullptr,
                                        double* r3sq = nullptr) {
  return phase_a_core<FAST, ROT, ZEXT, NOWALL, WORD, RTAB, CFG>(H, P, L, uniforms_of(seed_lo, seed_hi, ray_id, u3_hi), st, sampled, reached, radial, M, held, r3sq);
}

// z of pointExitCB in the rotated telescope frame (z0 of :2051) from the ray as phase B knows it: the point of the ray whose z
// *before* the rotation (rotateInY(rotateInX(.)) about (0, 0, lT/2), :1888-1894) is -Lp.  With m = third column of that rotation
// and q(Z) = (qx + tsx Z, qy + tsy Z, Z), qx / qy = X0 / Y0 + entrance offset:  m . (q - c) + lT/2 = -Lp, linear in Z.
__device__ __forceinline__ double zcb_rotated(double mx, double my, double mz, double h, double qx, double qy, double tsx, double tsy, double Lp) {
  const double num = -Lp - h - fma(mx, qx, fma(my, qy, -mz * h));
  return num * frcp(fma(mx, tsx, fma(my, tsy, mz)));
}

// Results of phase B for one ray (record mode needs all of them; histogram mode a few).
struct RayOut {
  // lane masks (ballots taken where the predicates are computed: a bool carried across basic blocks is materialised as a
  // per-lane 0 / 1 and compared again)
  uint64_t m_nickel = 0, m_till = 0, m_passed = 0;
  bool passed = false;      // finished && weight != 0
#ifdef SART_STAGE_TIMING
  uint64_t tb[6] = {0, 0, 0, 0, 0, 0};
#endif
  double px = 0.0, py = 0.0, rdet = 0.0, weight = 0.0, reflect = 0.0;
  int e_idx = 0;
  GasRay gas = {0.0, 0.0, 0.0, 0.0, 0.0};   // SCAN: what the per-mass conversion probability needs of this ray
};

// ------------------------------------------------------------------------------------------------
// phase B: mirrors -> detector plane -> weights -> window (:1971-2221), predicated like phase A:
// `live` carries the reference's early returns.  Dead lanes keep computing (indices are clamped so that
// every table access stays in range); only record fields and the final outputs look at `live`.
// ------------------------------------------------------------------------------------------------
// GAS: stage known at compile time (0 vacuum / 1 gas) or read at run time (-1).  ZEXT: see phase_a.
// SCAN (fused mass scan): the gas-stage conversion probability is left out - out.weight is the mass-independent factor of the
// weight, out.gas what gas_conversion_prob() needs of this ray, out.m_passed the rays on the chip for which that factor is not
// zero; the caller applies the probability per mass.
// NODRAW: the caller always hands the energy index in (fused angular scan: drawn once per ray in front of the angle loop).
// ESCAN (fused energy scan, X-ray test source): phase B stops once the geometry is known - mirrors, reflection-angle cells,
// detector plane, chip and strips - and hands what the weight needs of the ray to the caller in *geo (EScanGeo); no energy row,
// no reflectivity gather, no weight.  out.m_nickel is set as usual.
// 1: phase B of the accumulating kernels gathers the energy row and the reflectivities for live lanes only (0: for every lane;
// experiment builds)
#ifndef SART_GATHER_LIVE
#define SART_GATHER_LIVE 1
#endif
// 1: ... and everything behind the gathers - detector plane, chip and strip geometry, weights, out.* - runs for those lanes only
// (0: only the three gathers are predicated; experiment builds).  The record kernel and the energy scan keep the flat form.
#ifndef SART_B_LIVE_REGION
#define SART_B_LIVE_REGION 1
#endif
// 1: trace_histogram_kernel holds phase A's sine / cosine coefficients in vector registers where it has them to spare (0: every
// pass writes them into scalar registers; experiment builds)
#ifndef SART_A_SINCOS_VGPR
#define SART_A_SINCOS_VGPR 1
#endif
struct EScanGeo {
  double cos_ya, path_cb, distance_pipe_m, xu1, xu2;
  int ia1, ia2;
  uint64_t m_live;      // rays alive behind the mirrors (the lanes N_PASSED_TILL_WINDOW counts, given a non-zero weight)
  uint64_t m_chip;      // ... and on the chip (the lanes N_PASSED counts, given a non-zero final weight)
  uint64_t m_strip;     // rays inside a strongback strip
};
// CFG: HistCfg - how the wave-uniform switches are answered (RunTimeCfg: read per pass; FoldedCfg: constants).
template <bool RECORDS, bool FAST, int GAS, bool ZEXT, bool SCAN = false, bool NODRAW = false, bool ESCAN = false, class CFG = RunTimeCfg>
__device__ __forceinline__ void phase_b(const DevParams& P, const LdsTables& L, const HotB& HB, const TraceArgs& A,
                                        const RayState& st, int e_idx_in, bool live, RayOut& out, sart_axion_t* rec,
                                        EScanGeo* geo = nullptr) {
#ifdef SART_STAGE_TIMING
#define SART_B_STAMP(k, dep) do { asm volatile("" :: "v"(dep)); out.tb[k] = __builtin_readcyclecounter(); } while (0)
#else
#define SART_B_STAMP(k, dep)
#endif
  SART_B_STAMP(0, st.X0);
  // the accumulating kernels draw with the ray's own random word (st.u5_hi: u5 = u5_hi / 2^32); the record kernel may have been
  // handed its uniforms from outside and keeps the general draw
  constexpr bool WORD = !RECORDS;
  // the energy draw runs beside the mirror arithmetic (its gathers are issued early, consumed late)
  const bool draw_energy = NODRAW ? false : __builtin_amdgcn_readfirstlane(e_idx_in) < 0;   // wave-uniform: false for the X-ray test source
  EnergyDraw ed;   // (no initialiser: a field one form of the draw leaves unwritten would carry its zero across that form's branch)
#ifdef SART_DEBUG_KNOBS
  // working-set experiments (wrong results by design): 0x04000000 guide rows folded onto 16, 0x02000000 CDF rows folded onto 16,
  // 0x01000000 reflectivity / energy rows folded onto 32
  const uint32_t dbg = (uint32_t)__builtin_amdgcn_readfirstlane((int)A.flags);
  if (draw_energy) energy_draw_begin<WORD, CFG>(HB, (dbg & 0x02000000u) ? (st.r_idx & 15) : st.r_idx, st.u5, st.u5_hi, ed, (dbg & 0x04000000u) ? (st.r_idx & 15) : st.r_idx);
#else
  if (draw_energy) energy_draw_begin<WORD, CFG>(HB, st.r_idx, st.u5, st.u5_hi, ed);
#endif
  const ShellDev& sh = L.shells[st.shell];
  // P / A may live in LDS: branch conditions are made wave-uniform (scalar branches) explicitly.
  // FAST: vacuum stage, solar source (known at compile time).
  const int wolter = CFG::kFoldB ? CFG::kWolter : __builtin_amdgcn_readfirstlane(P.telescope_wolter);
  static_assert(!ZEXT || GAS >= 0, "the z-extent form needs the stage at compile time");
  static_assert(!SCAN || !RECORDS, "the mass scan accumulates, it writes no records");
  const int stage_gas = (GAS >= 0) ? GAS : __builtin_amdgcn_readfirstlane(P.stage_gas);
  const int test_active = FAST ? 0 : __builtin_amdgcn_readfirstlane(P.test_active);
  const int n_half_strips = CFG::kFoldStrips ? CFG::kHalfStrips : __builtin_amdgcn_readfirstlane(P.n_half_strips);
  // (folded: every test of a bit of kFoldedFlags is then a constant)
  const uint32_t flags = CFG::kFoldB ? (uint32_t)__builtin_amdgcn_readfirstlane((int)A.flags) & ~kFoldedFlags : (uint32_t)__builtin_amdgcn_readfirstlane((int)A.flags);
  const double X0 = st.X0, Y0 = st.Y0, tsx = st.tsx, tsy = st.tsy, zcb = st.zcb;
  const double Q0 = fma(X0, X0, Y0 * Y0);

  // ---- mirror 1 (:1985-1992 / :2012-2019) ----
  const double D0 = fma(X0, tsx, Y0 * tsy);
  const double A0 = fma(tsx, tsx, tsy * tsy);
  const double L0 = 1.0 + A0;                 // |w|^2 of the un-normalised direction w = (tsx, tsy, 1)
  double z1;
  uint64_t live_m = ballot64(live), hit1_m, hit2_m;   // `live` and the cuts below as lane masks, combined on the scalar unit
  const bool hit1 = pick_root(A0 - sh.m1_k, D0 + sh.m1_hb, Q0 - sh.m1_cc, 0.0, sh.m1_zhi, z1, hit1_m);
  if (!hit1) z1 = zcb;                        // the reference returns its input point (:656-658)
  const double m1x = fma(z1, tsx, X0), m1y = fma(z1, tsy, Y0);
  // on the surface the normal's z-component is closed-form: cone tan(b) rho(z); paraboloid r3 tan(b)
  double n1z = wolter ? sh.n1_r3t : sh.n1_tan * fma(-sh.n1_tan, z1, sh.r1);
  if (live & !hit1)                           // divergent, skipped when no lane needs it: the normal at the (off-surface) input point
    n1z = normal_z_general(P, sh, 1, m1x, m1y, z1);
  if (draw_energy) energy_draw_candidates<WORD, CFG>(HB, ed);   // the guide word has had the first mirror's arithmetic to arrive
  double wx = tsx, wy = tsy, wz = 1.0;
  const double N1 = fma(m1x, m1x, fma(m1y, m1y, n1z * n1z));
  double sin_a1, sin_a2;
  const double sin2_a1 = reflect(wx, wy, wz, L0, m1x, m1y, n1z, N1, sin_a1);

  // lineHitsNickel (:1706-1734), evaluated before the no-hit test (:2040-2057):
  // tan(a1) > num / (l - z1)  <=>  sin^2(a1) ((l - z1)^2 + num^2) > num^2   (num >= 0, l - z1 > 0)
  {
    const double lz = P.l_mirror - z1, num = sh.nickel_num;
    bool nick = sin2_a1 * fma(lz, lz, num * num) > num * num;
    uint64_t nick_m = ballot64(nick);
    if (ballot64(!(lz > 0.0))) {               // wave-uniform; only for a missed mirror with z1 >= l (never in practice)
      if (!(lz > 0.0)) nick = fsqrt(sin2_a1 / (1.0 - sin2_a1)) > num / lz;
      nick_m = ballot64(nick);
    }
    const bool upper = st.shell > 0;
    const bool hit_nickel = live & upper & nick;
    out.m_nickel = live_m & ballot64(upper) & nick_m;
    if (RECORDS && hit_nickel) rec->hitNickel = 1;
    live = live & !hit_nickel & hit1;         // nickel (:2045), almostEqual(z1, z0) (:2055)
    live_m = live_m & ~out.m_nickel & hit1_m;
  }

  SART_B_STAMP(1, wz);
  // ---- mirror 2 (:1994-2001 / :2021-2028): ray through (m1x, m1y, z1) along w ----
  const double inv_wz = frcp(wz);
  const double s2x = wx * inv_wz, s2y = wy * inv_wz;
  const double X1 = fma(-z1, s2x, m1x), Y1 = fma(-z1, s2y, m1y);   // extrapolated to z = 0
  const double A1 = fma(s2x, s2x, s2y * s2y);
  const double D1 = fma(X1, s2x, Y1 * s2y);
  const double Q1 = fma(X1, X1, Y1 * Y1);
  double z2;
  const bool hit2 = pick_root(A1 - sh.m2_k, D1 + sh.m2_hb, Q1 - sh.m2_cc, sh.m2_zlo, sh.m2_zhi, z2, hit2_m);
  live = live & hit2;                         // almostEqual(z1, z2) (:2055)
  live_m &= hit2_m;
  if (!hit2) z2 = sh.m2_zlo;
  const double m2x = fma(z2, s2x, X1), m2y = fma(z2, s2y, Y1);
  const double n2z = wolter ? sh.n2_r3t * fma(2.0 * (P.l_mirror - z2), sh.n2_invF, 1.0)
                            : sh.n2_tan * fma(-sh.n2_tan, z2 - sh.m2_zlo, sh.m2_rc);
  const double N2 = fma(m2x, m2x, fma(m2y, m2y, n2z * n2z));
  const double sin2_a2 = reflect(wx, wy, wz, L0, m2x, m2y, n2z, N2, sin_a2);

  SART_B_STAMP(2, wz);
  // ---- reflectivity lookups, angle part (computeReflectivity :1533-1580: bilinear in (angle, energy); the energy
  // interpolation is folded into the per-energy-index table, leaving a linear interpolation in the angle).  The cell and
  // the fraction inside it do not depend on the energy index: computed while the CDF candidates are in flight ----
  const bool use_refl = !(flags & SART_CF_IGNORE_REFLECTION);
  int ia1 = 0, ia2 = 0;
  double xu1 = 0.0, xu2 = 0.0;
  if (use_refl) {
    const int na2 = HB.refl_n_angles - 2;
    const double amin = P.refl_angle_min, inv_da = P.refl_inv_dangle, da = P.refl_dangle;
    double asin_a1, asin_a2;
    asin_small_pair(sin_a1, sin2_a1, sin_a2, sin2_a2, asin_a1, asin_a2);   // getMirrorAngle (:782-795) of both mirrors
    auto angle_cell = [&](double asin_a, double& xu_out) {
      // alpha = asin_a * 57.29577951308232 (degrees), and both differences alpha - x as ONE fused operation each: what the
      // compiler's contraction made of `alpha - x` in every instantiation.  Written out, because the contraction pass decides per
      // basic block: with the folded form's one block around this arithmetic it kept the product apart - an ulp in xu.
      constexpr double kDeg = 57.29577951308232;
      const double t = fma(asin_a, kDeg, -amin) * inv_da;
      int i = (int)t;                 // = floor(t) for t >= 0; negative or NaN t ends in cell 0 through the clamp
      i = max(min(i, na2), 0);
      xu_out = fma(asin_a, kDeg, -fma((double)i, da, amin)) * inv_da;
      return i;
    };
    ia1 = angle_cell(asin_a1, xu1);
    ia2 = angle_cell(asin_a2, xu2);
  }

  // ---- energy index; the energy row and the two reflectivity pairs are requested the moment it is known and consumed
  // behind the detector-plane and window geometry ----
#ifdef SART_DEBUG_KNOBS
  const int e_idx = (dbg & 0x01000000u) ? ((draw_energy ? energy_draw_finish<WORD, CFG>(HB, ed) : e_idx_in) & 31) : (draw_energy ? energy_draw_finish<WORD, CFG>(HB, ed) : e_idx_in);
#else
  const int e_idx = draw_energy ? energy_draw_finish<WORD, CFG>(HB, ed) : e_idx_in;
#endif
  SART_B_STAMP(3, e_idx);
  // Accumulating kernels: only the lanes whose ray is still alive behind both mirrors (nickel, no-hit tests: `live` is settled
  // here; lanes beyond the pass' valid rays included) go on - `live_m` discards whatever the others would compute, so they are
  // switched off from here to the end of the function (REGION: ONE predicated region, skipped by a wave without a live lane).
  // What leaves the region per lane (the r_* values and out.* below) is left UNSPECIFIED for the dead lanes instead of
  // defaulted - a default is a v_mov per register at the join.  The compares and ballots behind out.m_till / out.m_passed stay
  // behind the region, on those values, and keep their `live_m &`: a mask written inside it would be a per-lane value at the
  // join (the compiler turns a predicate that crosses it into v_cndmask + v_cmp per ballot).  Record mode and the energy scan run
  // flat, for every lane, with every default.
  constexpr bool REGION = SART_B_LIVE_REGION && SART_GATHER_LIVE && !RECORDS && !ESCAN;
  const bool gather = (RECORDS || !SART_GATHER_LIVE) ? true : __builtin_amdgcn_inverse_ballot_w64(live_m);
  // (wave-uniform: the gas stage's conversion probability is multiplied in last, a zero takes the ray out of out.m_till)
  const bool r_prob_deferred = REGION && !SCAN && stage_gas != 0 && !(flags & SART_CF_IGNORE_CONV_PROB);
  // (deliberately without initialisers: an initial value is what the dead lanes would carry across the join.  Every lane reads
  // them behind the region - through the empty asm there, so that nothing is derived from "unwritten" - and live_m or
  // out.m_passed masks whatever a dead lane holds.)
  double r_pdx, r_pdy, r_rdet2, r_w_till, r_weight, r_reflect, r_prob;
  GasRay r_gas;
  out.e_idx = e_idx;
  // (the body keeps the function's indentation: it is the function's tail, called under `gather` or unconditionally)
  auto behind_the_mirrors = [&]() __attribute__((always_inline)) {
  if constexpr (REGION) asm volatile("; hot: phase B behind the mirrors, live lanes only");
  EnergyDev en = {};
  d2 g1 = {1.0, 1.0}, g2 = {1.0, 1.0};
  if (!ESCAN && (REGION || gather)) {
    asm volatile("; hot: gathers of the live lanes");
    en = load_energy_row(HB, e_idx);
    if (use_refl) {
      // row (coating, e_idx) of refl[][n_angles]: 32-bit element offset (the table is < 4 GB, checked on the host)
      const uint32_t row = __umul24((uint32_t)(sh.refl_row0 + e_idx), (uint32_t)HB.refl_n_angles);
      g1 = gload<d2>(HB.refl, (row + (uint32_t)ia1) * 8u);   // g[i], g[i + 1] (8-byte aligned pair)
      g2 = gload<d2>(HB.refl, (row + (uint32_t)ia2) * 8u);
    }
  }

  // ---- detector plane: getPointDetectorWindow (:797-814, :2070-2083) ----
  const double pmx = fma(m2x, P.pipe_c, z2 * P.pipe_s) - P.d_cb_xray;
  const double pmz = fma(z2, P.pipe_c, -m2x * P.pipe_s);
  const double vx = fma(wx, P.pipe_c, wz * P.pipe_s);
  const double vz = fma(wz, P.pipe_c, -wx * P.pipe_s);
  const double inv_vz = frcp(vz);
  const double nwin = (sh.dist_det - pmz) * inv_vz;
  double pdx = fma(nwin, vx, pmx), pdy = fma(nwin, wy, m2y), pdz = sh.dist_det;

  // yaw angle (:2101-2115): ya = deg(atan2(-v_z, -v_y)) + 90 = -deg(atan(v_y / v_z)); only its cosine is used unless
  // the record is written
  const double ya = RECORDS ? -atan_small(tsy) * 57.29577951308232 : 0.0;
  const double cos_ya = RECORDS ? cos_small(ya) : cos_yaw_of_slope(tsy);

  if (RECORDS && live) {
    const double nend = (sh.dist_det_end - pmz) * inv_vz;
    const double ddx = (nend - nwin) * vx, ddy = (nend - nwin) * wy;
    rec->deviationDet = sqrt(fma(ddx, ddx, ddy * ddy));           // :2085-2088
    rec->pointdataXBefore = X0;                                    // :2091-2094
    rec->pointdataYBefore = Y0;
    rec->pixvalsX = floor(X0 / (48.0 / 1400.0)) + 700.0;           // getPixelValue (:618-623)
    rec->pixvalsY = floor(Y0 / (48.0 / 1400.0)) + 700.0;
  }

  const double distance_pipe_m = (pdz - zcb) * 1e-3;               // :2116 (before the straight-through override of pdz)
  if (test_active) {   // straight through the hole in the optics (:2130-2132)
    const bool through = (sh.r1 - fsqrt(Q0)) > 100.0;
    pdx = through ? fma(sh.dist_det_raw, tsx, X0) : pdx;
    pdy = through ? fma(sh.dist_det_raw, tsy, Y0) : pdy;
    pdz = through ? sh.dist_det_raw : pdz;
  }
  pdx -= P.lateral_shift;
  pdy -= P.transversal_shift;

  // ---- geometry of the detector window / chip (:2138-2147) and of the window strips (:2149-2187: rotateAroundZ by theta,
  // strips along x): none of it needs the gathers, so it runs before they are consumed ----
  const double rdet2 = fma(pdx, pdx, pdy * pdy);
  const bool off_window = rdet2 > P.radius_window_sq, off_x = fabs(pdx) > P.chip_cx, off_y = fabs(pdy) > P.chip_cy;
  const bool on_chip = !((!(flags & SART_CF_IGNORE_DET_WINDOW)) & off_window) & !(off_x | off_y);
  const uint64_t on_chip_m = REGION ? 0ull : ~(((flags & SART_CF_IGNORE_DET_WINDOW) ? 0ull : ballot64(off_window)) | ballot64(off_x) | ballot64(off_y));
  if constexpr (REGION) { r_pdx = pdx; r_pdy = pdy; r_rdet2 = rdet2; }
  const double yt = fabs(fma(pdy, P.theta_c, -pdx * P.theta_s));
  bool in_strip = false;
  for (int i = 0; i < n_half_strips; ++i) in_strip = in_strip | ((yt > P.strip_lo[i]) & (yt < P.strip_hi[i]));
  if constexpr (ESCAN) {
    static_assert(!RECORDS && !SCAN && !FAST, "the energy scan accumulates, and it runs on the generic variants");
    geo->cos_ya = cos_ya;
    geo->path_cb = st.path_cb;
    geo->distance_pipe_m = distance_pipe_m;
    geo->xu1 = xu1; geo->xu2 = xu2;
    geo->ia1 = ia1; geo->ia2 = ia2;
    geo->m_live = live_m;
    geo->m_chip = live_m & on_chip_m;
    geo->m_strip = ballot64(in_strip);
    (void)en; (void)g1; (void)g2; (void)on_chip;
    return;
  }

  // ---- weights (:2116-2128) ----
  const double path_cb = st.path_cb;
  double trans_magnet;
  // Gas stage, accumulating kernels: the conversion probability is the one factor that depends on the axion mass; it is
  // applied LAST (below; per mass by the caller when SCAN), trans_magnet goes without it.  Wave-uniform.
  bool prob_deferred = false;
  {
    double prob = 1.0;
    double absorb = 1.0;
    if (!stage_gas) {
      // conversionProb (:363-365) = conv_k pathCB^2; FAST carries the z extent of the path: pathCB^2 = z^2 (1 + slope^2)
      if (!(flags & SART_CF_IGNORE_CONV_PROB)) prob = ZEXT ? (P.conv_k * L0) * (path_cb * path_cb) : P.conv_k * path_cb * path_cb;
    } else {
      // axionConversionProb2 / intensitySuppression2 (axionMassforMagnet.nim:75-113) with pathCB as length
      const double path_len = ZEXT ? path_cb * fsqrt_pos(L0) : path_cb;   // ZEXT: the ring carries the z extent of the path
      const double Lnat = path_len * P.gas_inv_hbarc_m;              // length / 1.97e-7, length in m
      if (!(flags & SART_CF_IGNORE_CONV_PROB)) {
        const double g = en.gamma;
        const double eh = exp_neg(-g * Lnat * 0.5);                    // exp(-Gamma L) = eh^2: one exp for both terms
        out.gas = GasRay{en.inv_two_e_ev, g * g * 0.25, -2.0 * eh, fma(eh, eh, 1.0), Lnat};
        if (RECORDS) prob = gas_conversion_prob(P.gas_dm2_abs, out.gas, P.gas_term1, L.sincos, GasCos::make());
        else prob_deferred = true;
      }
      // intensitySuppression2 (axionMassforMagnet.nim:100-113): exp(-mu_pipe d) exp(-mu_magnet L) as one exponential
      absorb = exp_neg(-fma(en.mu_pipe, distance_pipe_m, en.mu_magnet * (path_len * 1e-3)));
    }
    trans_magnet = cos_ya * prob * absorb;          // cos of a degree value taken as radians — sic (:1598)
  }
  // R(alpha, E_idx) = g[i] + xUnit (g[i + 1] - g[i]) for both mirrors (with ignoreReflection: g = (1, 1))
  const double reflectv = fma(xu1, g1.y - g1.x, g1.x) * fma(xu2, g2.y - g2.x, g2.x);
  double weight = reflectv * trans_magnet;
  SART_B_STAMP(4, weight);
  if (RECORDS && live) {
    rec->transmissionMagnet = trans_magnet;
    rec->yawAngles = ya;
    rec->reflect = reflectv;
  }

  const bool has_weight = weight != 0.0;
  const bool till_window = live & has_weight;
  if constexpr (REGION) r_w_till = weight;
  else out.m_till = live_m & ballot64(has_weight);   // (a deferred conversion probability of exactly zero is taken out below)
  if (RECORDS && till_window) rec->passedTillWindow = 1;
  live = live & on_chip;
  if constexpr (!REGION) live_m &= on_chip_m;

  const double trans_window = (n_half_strips > 0) ? (in_strip ? en.t_strongback : en.t_window) : 0.0;
  const uint8_t kind_w = in_strip ? SART_MK_SI : SART_MK_SI3N4;
  // wave-uniform switches as scalar branches around one multiplication each (the empty asm keeps LLVM from turning them
  // into a multiplication plus a two-instruction select that every launch pays)
  if (!(flags & SART_CF_IGNORE_DET_WINDOW)) { asm volatile(""); weight *= trans_window; }
  if (!(flags & SART_CF_IGNORE_GAS_ABS)) { asm volatile(""); weight *= en.a_gas; }        // :2190-2192
  if (!(flags & SART_CF_XRAY_TEST)) { asm volatile(""); weight *= P.exposure; }           // :2207-2212
  if (!SCAN && prob_deferred) {
    const double prob = gas_conversion_prob(P.gas_dm2_abs, out.gas, P.gas_term1, L.sincos, GasCos::make());
    weight *= prob;
    if constexpr (REGION) r_prob = prob;
    else out.m_till &= ballot64(prob != 0.0);
  }

  SART_B_STAMP(5, weight);
  const bool final_weight = weight != 0.0;
  if constexpr (!REGION) {
    out.m_passed = live_m & ballot64(final_weight);
    out.passed = RECORDS ? (live & final_weight) : __builtin_amdgcn_inverse_ballot_w64(out.m_passed);
  }
  if constexpr (REGION) {
    r_reflect = reflectv; r_weight = weight;
    if constexpr (SCAN) r_gas = out.gas;
  } else {
    out.reflect = reflectv;
    out.rdet = fsqrt_pos(rdet2 + 1e-300);     // + 1e-300: exact no-op unless the ray hits the chip centre to the last bit
    out.weight = weight;
  }
  if constexpr (!REGION) {
    out.px = -pdx + P.chip_cx;                                        // :2203-2204
    out.py = pdy + P.chip_cy;
  }
  if (RECORDS && live) {
    if (n_half_strips > 0) {
      rec->transProbWindow = trans_window;
      rec->energiesAxWindow = en.energy;
      rec->kindsWindow = kind_w;
    }
    rec->transProbArgon = en.a_gas;
    rec->transProbDetector = en.a_gas;
    rec->energiesAxAll = en.energy;
    rec->kinds = SART_MK_AR;
    rec->energiesAx = en.energy;
    rec->shellNumber = st.shell;
    rec->pointdataR = out.rdet;
    rec->pointdataX = out.px;
    rec->pointdataY = out.py;
    rec->weights = weight;
    rec->weightsAll = weight;
    rec->passed = (weight != 0.0) ? 1 : 0;
  }
  };   // behind_the_mirrors
  if constexpr (REGION) {
    // (a copy of the flags that the region does not share: a test of `flags` made on both sides of the join is merged into a
    // per-lane value across it)
    uint32_t flags_j = flags;
    asm volatile("" : "+s"(flags_j));
    if (gather) behind_the_mirrors();
    // (opaque: the compiler otherwise sinks the compares below into the region and carries their predicates across the join)
    asm volatile("" : "+v"(r_pdx), "+v"(r_pdy), "+v"(r_rdet2), "+v"(r_w_till), "+v"(r_weight));
#ifdef SART_STAGE_TIMING
    // Stamps 4 and 5 are taken inside the region.  A value assigned under a lane mask is a per-lane value behind the join: the dead
    // lanes keep the initial zero - lane 0, whose sums the epilogue stores, among them - and a wave without a live lane skips both
    // stamps (span 4 = 0 - stamp 3, a number near 2^64 in every such pass).  Both are read back from the first live lane; without one
    // the region did not run and its two sub-stages are empty: both stamps are stamp 3.
    {
      const int src = live_m ? (int)__builtin_ctzll(live_m) : 0;
      for (int k = 4; k < 6; ++k) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)out.tb[k], src);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(out.tb[k] >> 32), src);
        out.tb[k] = live_m ? ((uint64_t)hi << 32 | lo) : out.tb[3];
      }
    }
#endif
    // the region's predicates and their masks, with every lane switched on again, as the flat form takes them: the dead
    // lanes' bits are unspecified and fall to live_m (still the rays alive behind the mirrors)
    out.m_till = live_m & ballot64(r_w_till != 0.0);
    if (r_prob_deferred) out.m_till &= ballot64(r_prob != 0.0);
    const uint64_t off_m = ((CFG::kFoldB ? 0u : flags_j & SART_CF_IGNORE_DET_WINDOW) ? 0ull : ballot64(r_rdet2 > P.radius_window_sq)) | ballot64(fabs(r_pdx) > P.chip_cx) |
                           ballot64(fabs(r_pdy) > P.chip_cy);
    out.m_passed = live_m & ~off_m & ballot64(r_weight != 0.0);
    out.reflect = r_reflect; out.weight = r_weight;
    out.rdet = fsqrt_pos(r_rdet2 + 1e-300);   // (consumed by the passed rays only: the compiler sinks it into their region)
    if constexpr (SCAN) out.gas = r_gas;
    out.passed = __builtin_amdgcn_inverse_ballot_w64(out.m_passed);
    out.px = -r_pdx + P.chip_cx;                                      // :2203-2204
    out.py = r_pdy + P.chip_cy;
  } else {
    behind_the_mirrors();
  }
}

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
// Wave priorities by pipeline stage (s_setprio: the SIMD's arbiter picks the ready wave with the highest priority): the four
// persistent waves of a SIMD are in different stages at any moment, and the later the stage the sooner its instructions should
// go - a wave in phase B has three dependent table gathers to get into flight (everything it issues ahead of them is latency
// the others could have hidden), a wave in phase A feeds it, the accumulation behind phase B (atomics nobody waits for) and
// stage A0 are filler that runs whenever nobody else can.  Priced in profiles/r05_exp_setprio.txt (same-box A/B of eleven
// assignments, bitwise the same results): B 3 > A1 2 > accumulation 1 > A0 / loop glue 0 is worth 9 % on BabyIAXO / XMM, 9 % on
// the gas stage and the rotated telescope, 8 % on CAST / LLNL against every wave at priority 0 (oldest first); what matters
// most is stage A0 below everything else (A1 = B = 1: 6 %), then B above A1 (+3 %).
#ifndef SART_PRIO_A1
#define SART_PRIO_A1 2
#endif
#ifndef SART_PRIO_B
#define SART_PRIO_B 3
#endif
#ifndef SART_PRIO_ACC
#define SART_PRIO_ACC 1
#endif
constexpr int kQueue = 128;   // ring capacity per wave: < 64 left over + <= 64 new survivors

struct __align__(16) TablesLds {
  double sincos[2 * kSinCosEntries];
  uint32_t rcdf_hi[kMaxRadii + 4];   // floor(fluxRadiusCDF 2^52) >> 20 = floor(cdf 2^32), saturated; + four entries of 1.0 behind the table (four-wide candidate read)
  ShellDev shells[kMaxShells];
  uint16_t rguide[kRadiusGuideEntries + 6];
  uint8_t lut[kShellLutMax];
};

// per-wave survivor rings (structure of arrays: lane i reads slot (head + i) % 128 -> conflict-free)
// One wave's rings side by side (7.7 KB): every field is then reachable from a single per-wave base address with an
// immediate offset, instead of one base register per array.
struct __align__(16) WaveRings {
  double X0[kQueue], Y0[kQueue], tsx[kQueue], tsy[kQueue];
  double path[kQueue], u5[kQueue];
  int idx[kQueue];                        // r_idx | shell << 16
  uint32_t ray[kQueue];                   // ring 0: rays that passed stage A0 (ray id relative to the launch's first chunk)
  uint32_t u3hi[kQueue];                  //         and their word of the shared stream (high word of u3)
};
// The rings of trace_histogram_kernel: ring 1 carries the energy draw's uniform as the 32-bit word it is made of (u5 = z / 2^32
// exactly, uniforms_of) in one 8-byte cell beside the packed indices - one LDS store and one LDS load per entry instead of two, and
// 512 bytes per wave less than WaveRings, which the image tile gets (sart_device.h: kTileExtraCells).  The other kernels keep
// WaveRings: their u5 column holds a workgroup's scan cells.
struct __align__(16) HistRings {
  double X0[kQueue], Y0[kQueue], tsx[kQueue], tsy[kQueue];
  double path[kQueue];
  uint2 cell[kQueue];                     // {r_idx | shell << 16, z}
  uint32_t ray[kQueue];                   // ring 0, as in WaveRings
  uint32_t u3hi[kQueue];
};
static_assert(sizeof(WaveRings) - sizeof(HistRings) == kQueue * sizeof(uint32_t) && sizeof(HistRings) % 512 == 0 &&
                  (kTileRingCells / kQueue * (sizeof(WaveRings) - sizeof(HistRings))) / sizeof(double) == kTileExtraCells + kRadialTableCells - kRingExtraCells,
              "what ring 1's packed cell frees is what the histogram kernels' image tile grows by");
template <int WAVES, typename Rings = WaveRings>
struct __align__(16) QueueLds {
  Rings w[WAVES];
};

// `radial_cells`: the look-up table gets the cells of the radial verdict table instead of the shell selection's own
template <int BLOCK>
__device__ __forceinline__ void stage_tables(TablesLds& S, const DevParams& P, const DevTables& T, bool radial_cells = false) {
  for (int i = threadIdx.x; i < 2 * kSinCosEntries; i += BLOCK) S.sincos[i] = as_global(T.sincos_tab)[i];
  for (int i = threadIdx.x; i < P.n_radii + 4; i += BLOCK) {   // (cdf_hi32_kernel's definition, sart_tables.hip)
    const double c = (i < P.n_radii) ? as_global(T.flux_radius_cdf)[i] : 1.0;
    const unsigned long long t = __double2ull_rd(c * 4503599627370496.0) >> 20;   // floor(cdf 2^32); the product is exact: cdf <= 1
    S.rcdf_hi[i] = t > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)t;
  }
  for (int i = threadIdx.x; i < kRadiusGuideEntries; i += BLOCK) S.rguide[i] = as_global(T.radius_guide)[i];
  {
    const auto src = as_global(reinterpret_cast<const uint64_t*>(T.shells));
    uint64_t* dst = reinterpret_cast<uint64_t*>(S.shells);
    const int n = P.n_shells * (int)(sizeof(ShellDev) / 8);
    for (int i = threadIdx.x; i < n; i += BLOCK) dst[i] = src[i];
  }
  const uint8_t* lut = T.shell_lut + (radial_cells ? kRadialCellsOffset : 0);
  for (int i = threadIdx.x; i < P.lut_n; i += BLOCK) S.lut[i] = as_global(lut)[i];
  __syncthreads();
}

// Fused trace + accumulate (traceAxionWrapper + prepareHeatmap + flux sum + counters) as a three-stage
// pipeline inside one persistent wave, with wavefront compaction (ballot + prefix count into per-wave LDS
// rings) between the stages:
//   A0  word of the shared stream -> radius of the point on the bore exit -> provably dead rays leave (HotA zones)
//   A1  phase A (full sampling + cuts + shell selection) on full waves of A0 survivors
//   B   phase B (mirrors + weights + accumulation) on full waves of A1 survivors
// Rays are taken in chunks of 256 consecutive global ids, aligned to 256: lane l of the wave that owns a chunk handles
// ids 4l .. 4l+3 of it in four successive passes, so that the one block of the shared word stream it computes (stage A0's
// only Philox block) serves all four.  Ray i of this launch has the global id ray_id_offset + i; n_rays < 2^31 per launch.
// FAST: solar source, vacuum, no hole loop, telescope not rotated (all known at compile time).  ROT: rotated telescope
// (phase B then recomputes z of pointExitCB from the ray instead of carrying it through ring 1).
// Re-reads the HotA block (the first kernel argument) from the kernel-argument segment with scalar loads.  The pointer
// is laundered so that the loads stay where they are written (the start of a phase-A pass) instead of being hoisted
// out of the persistent loop: ~50 SGPRs held across stage B get spilled through VGPR lanes (v_readlane = VALU slots).
__device__ __forceinline__ void reload_hot(HotA& dst) {
  typedef const __attribute__((address_space(4))) uint32_t* kernarg_ptr;
  kernarg_ptr p = (kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  uint32_t* d = reinterpret_cast<uint32_t*>(&dst);
#pragma unroll
  for (int k = 0; k < (int)(sizeof(HotA) / 4); ++k) d[k] = p[k];
}

// Same for the zone table of stage A0 (the tail of HotA): ten scalar registers that would otherwise be spilled and
// reloaded through VGPR lanes in every pass.
struct ZoneTable {
  int32_t n_zones;
  uint32_t zone_reached;
  uint32_t lo[kMaxZones], hi[kMaxZones];
};
static_assert(sizeof(ZoneTable) == sizeof(HotA) - offsetof(HotA, n_zones), "ZoneTable mirrors the tail of HotA");
static_assert(offsetof(WaveRings, u3hi) == offsetof(WaveRings, ray) + kQueue * sizeof(uint32_t) && offsetof(WaveRings, ray) % 8 == 0 &&
                  offsetof(HistRings, u3hi) == offsetof(HistRings, ray) + kQueue * sizeof(uint32_t) && offsetof(HistRings, ray) % 8 == 0,
              "the image tile uses ray + u3hi of every wave as 128 contiguous doubles");
__device__ __forceinline__ void reload_zones(ZoneTable& dst) {
  typedef const __attribute__((address_space(4))) uint32_t* kernarg_ptr;
  kernarg_ptr p = (kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(HotA, n_zones) / 4;
  asm volatile("" : "+s"(p));
  uint32_t* d = reinterpret_cast<uint32_t*>(&dst);
#pragma unroll
  for (int k = 0; k < (int)(sizeof(ZoneTable) / 4); ++k) d[k] = p[k];
}

// The argument block of trace_histogram_kernel as the code object lays it out (arguments in order, each at its natural
// alignment; tests/test_host_and_abi.py::test_kernel_argument_layout_matches_the_code_object compares these offsets with the
// code object's metadata on every run of the CPU suite).
struct HistKernArgs {
  HotA H;
  const DevBlob* blob;
  TraceArgs A;
  double* acc;
  HotB HB;
  ScanArgs SC;
};
static_assert(offsetof(HistKernArgs, H) == 0 && offsetof(HistKernArgs, blob) == (sizeof(HotA) + 7) / 8 * 8 &&
                  offsetof(HistKernArgs, A) == offsetof(HistKernArgs, blob) + 8 &&
                  offsetof(HistKernArgs, acc) == offsetof(HistKernArgs, A) + sizeof(TraceArgs) &&
                  offsetof(HistKernArgs, HB) == offsetof(HistKernArgs, acc) + 8 &&
                  offsetof(HistKernArgs, SC) == offsetof(HistKernArgs, HB) + sizeof(HotB) && sizeof(HotA) % 4 == 0 &&
                  sizeof(TraceArgs) % 8 == 0 && sizeof(HotB) % 8 == 0,
              "reload_hot / reload_zones / reload_kernarg read the arguments at these offsets");
// Re-reads one argument (or a leading part of it) from the kernel-argument segment with scalar loads at the place of use.
template <typename T>
__device__ __forceinline__ void reload_kernarg(T& dst, size_t byte_offset) {
  static_assert(sizeof(T) % 4 == 0, "dword granularity");
  typedef const __attribute__((address_space(4))) uint32_t* kernarg_ptr;
  kernarg_ptr p = (kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr() + byte_offset / 4;
  asm volatile("" : "+s"(p));
  uint32_t* d = reinterpret_cast<uint32_t*>(&dst);
#pragma unroll
  for (int k = 0; k < (int)(sizeof(T) / 4); ++k) d[k] = p[k];
}

// Instantiations: <FAST, ROT, GAS> = <true, false, 0> the common configuration; <true, false, 1> gas stage (the m_a scan of
// BASELINE configs[4]); <true, true, 0> rotated telescope (the angular scan of configs[3]); <false, *, -1> everything else
// (X-ray test source, hole loop, rotated + gas) with the switches read at run time.
// PATHC (common configuration only): the host has proved that no ray that survives phase A entered through the bore wall
// (sart_api.hip: build_zones), so the path in the magnetic field is the constant lengthB for every ray of phase B: ring 1
// does not carry it, and its 128 doubles per wave hold the LDS image tile instead (with stage A0 running beside it).
// FIXED: SART_ACCUM_FIXED64 - every sum is accumulated as an integer multiple of its quantum (to_fixed), with integer
// atomics in LDS and global memory; the slots of the replicas, of the partials and of the accumulator then hold int64.
// SCAN: fused axion-mass scan (sart_trace_mass_scan).  Stage B leaves the gas-stage conversion probability out of the weight and
// a loop over the launch's masses (ScanArgs: kernel arguments, read with scalar loads) applies it per mass:
// sum of w and of w^2 go to per-lane accumulators [mass][2][64] in the 16 KB of LDS that hold the image tile otherwise (ds_add_f64 /
// ds_add_u64 across the 16 waves of the workgroup); no image, no position sums.  Without PATHC that space is ring 0, so stage
// A0 stays off for such a launch whatever zones the host built.
// BANDS (SCAN only; mass_scan_spectra_kernel): the banded mass scan (sart_trace_mass_scan_spectra).  The 32 cells of a mass and
// quantity mean "energy band of the ray" instead of "lane % 32": cell b < n_bands is band b, cell n_bands everything outside the
// window.  The band comes from out.e_idx once per ray, in front of the per-mass loop; a u32[32] beside scan_zero counts the rays of
// out.m_passed per band.  The epilogue stores the workgroup's 64 cells per mass and the counts (fold_scan_bands_kernel) and, as
// without BANDS, their sums per mass (fold_scan_kernel: in FIXED the integers the plain scan stores).
// Room of a FIXED cell: it can now receive EVERY ray of the workgroup in a launch - at most 2^31 / 256 = 2^23 on the 256 workgroups
// of a full grid.  Sum of w: a ray adds < 2^(63 - headroom) quanta, 2^23 x 2^36 = 2^59 at the default headroom of 27; the host
// refuses a launch whose rays per workgroup exceed 2^(headroom - 1) (the cell would pass 2^62).  Sum of w^2: its quantum
// 2^(2 e' - 39), w_bound < 2^e', gives a ray < 2^39 quanta, so 2^23 rays of one workgroup stay below 2^62 - the room include/sart.h
// ("accumulation mode") promises for the rays of one workgroup of one launch, with nothing to spare: the host refuses more.
// (The body is sart_trace_histogram.inc: the banded scan's kernel, which needs a name of its own, shares the text.)
template <int BLOCK, bool FAST, bool ROT, int GAS, bool PATHC, bool FIXED, bool SCAN = false>
__global__ __launch_bounds__(BLOCK) void trace_histogram_kernel(HotA H, const DevBlob* __restrict__ blob, TraceArgs A,
                                                                double* __restrict__ acc, HotB HBarg, ScanArgs SCarg) {
  constexpr bool BANDS = false;
  using CFG = RunTimeCfg;
#include "sart_trace_histogram.inc"
}
// The folded form of the constant-path variants 5 (GAS 0) and 6 (GAS 1): the same body with FoldedCfg - the wave-uniform switches
// whose answers the reference's default configuration fixes are constants (HistCfg).  The host launches it only where every one of
// those answers holds (sart_device.h: folded_form_applies); same arguments, same offsets in the argument segment.
template <int BLOCK, int GAS, bool FIXED>
__global__ __launch_bounds__(BLOCK) void folded_histogram_kernel(HotA H, const DevBlob* __restrict__ blob, TraceArgs A,
                                                                 double* __restrict__ acc, HotB HBarg, ScanArgs SCarg) {
  constexpr bool FAST = true, ROT = false, PATHC = true, SCAN = false, BANDS = false;
  using CFG = FoldedCfg<GAS>;
#include "sart_trace_histogram.inc"
}
// The banded mass scan: the SCAN body with BANDS, under a name of its own (same arguments, same offsets in the argument segment).
template <int BLOCK, bool FAST, bool ROT, int GAS, bool PATHC, bool FIXED>
__global__ __launch_bounds__(BLOCK) void mass_scan_spectra_kernel(HotA H, const DevBlob* __restrict__ blob, TraceArgs A,
                                                                  double* __restrict__ acc, HotB HBarg, ScanArgs SCarg) {
  constexpr bool SCAN = true, BANDS = true;
  using CFG = RunTimeCfg;
#include "sart_trace_histogram.inc"
}

// ------------------------------------------------------------------------------------------------
// per-shell breakdown of the histogram trace (include/sart.h: sart_trace_histogram_shells_device)
// ------------------------------------------------------------------------------------------------
// trace_histogram_kernel's generic variants (stage read at run time, the path carried through ring 1; ROT: rotated telescope) with
// the same accumulator - image, scalars, spectra - plus, per shell, the counters and sums of the rays that selected it.  Shells
// differ from lane to lane, so those go to a per-workgroup table in LDS (ds_add_u32 for the counters, ds_add_f64 / ds_add_u64 for
// the sums) that is stored once per workgroup and folded by fold_shells_kernel; the per-shell energy spectra spread over
// n_shells x (n_energies + 1) slots and take global atomics like the existing spectra.  The table lives in the last
// kShellTableCells cells behind the tables, so the LDS image tile is at most kShellImageTileMax wide (host: sart_api.hip).
struct ShellKernArgs {
  HotA H;
  const DevBlob* blob;
  TraceArgs A;
  double* acc;
  HotB HB;
  ShellArgs SH;
};
static_assert(offsetof(ShellKernArgs, A) == offsetof(HistKernArgs, A) && offsetof(ShellKernArgs, HB) == offsetof(HistKernArgs, HB) &&
                  offsetof(ShellKernArgs, SH) == offsetof(HistKernArgs, SC),
              "the shell kernel shares the argument offsets of the histogram kernel");
static_assert(kShellImageTileMax * kShellImageTileMax <= kTileRingCells + kRingExtraCells - kShellTableCells &&
                  kShellImageTileExtraMax * kShellImageTileExtraMax <= kRingExtraCells - kShellTableCells,
              "the shell kernel's image tile leaves the shell table alone");

// ------------------------------------------------------------------------------------------------
// emission-channel breakdown of the histogram trace (include/sart.h: sart_trace_histogram_channels_device)
// ------------------------------------------------------------------------------------------------
// shell_histogram_kernel's twin: trace_histogram_kernel's generic variants with the same accumulator - image, scalars, spectra -
// plus, per channel t < T of the context's fraction table (ChannelArgs::frac, written by channel_fractions_kernel), the sums, the
// energy spectrum and the image of c_t = w f_t, where f is the run of `stride` doubles at (r_idx n_energies + e_idx) stride: r_idx
// travels through ring 1, e_idx comes out of phase B.  The run is ONE gather per passed ray (d2 loads of one aligned 64-byte line at
// most), requested under the live-lane mask of the passed rays in front of the accumulator's own arithmetic and atomics so that it
// flies behind them; the loop over t is wave-uniform (T from the kernel arguments) and unrolled, so f stays in registers.  Row sums
// and N_CONTRIBUTING go to per-workgroup LDS cells (kChanLanes cells each), summed and stored once per workgroup and folded by
// fold_channels_kernel; per-channel energy bins and pixels take global atomics like ascan_images_kernel's.  The table
// lives in the last kChanTableCells cells behind the tables, so the LDS image tile is at most kChanImageTileMax wide (host).
struct ChanKernArgs {
  HotA H;
  const DevBlob* blob;
  TraceArgs A;
  double* acc;
  HotB HB;
  ChannelArgs CH;
};
static_assert(offsetof(ChanKernArgs, A) == offsetof(HistKernArgs, A) && offsetof(ChanKernArgs, HB) == offsetof(HistKernArgs, HB) &&
                  offsetof(ChanKernArgs, CH) == offsetof(HistKernArgs, SC),
              "the channel kernel shares the argument offsets of the histogram kernel");

// ------------------------------------------------------------------------------------------------
// solar-origin map of the histogram trace (include/sart.h: sart_trace_histogram_origin_device)
// ------------------------------------------------------------------------------------------------
// The third user of the pipeline: the same accumulator plus, per passed ray, three global atomics (N, w, w^2) into the 32-byte cell
// (r_idx, e_idx) of the caller's map - r_idx travels through ring 1, e_idx comes out of phase B - issued under the live mask of the
// passed lanes behind the accumulator's own atomics.  The head of the block (N_PASSED and the two sums: what the cells must add up to)
// is the wave's own scalars, kept per wave in the last kOriginTableCells cells behind the tables, summed and stored once per workgroup
// and folded by fold_origin_kernel.
struct OriginKernArgs {
  HotA H;
  const DevBlob* blob;
  TraceArgs A;
  double* acc;
  HotB HB;
  OriginArgs OG;
};
static_assert(offsetof(OriginKernArgs, A) == offsetof(HistKernArgs, A) && offsetof(OriginKernArgs, HB) == offsetof(HistKernArgs, HB) &&
                  offsetof(OriginKernArgs, OG) == offsetof(HistKernArgs, SC),
              "the origin kernel shares the argument offsets of the histogram kernel");
static_assert(SART_ORIGIN_CELL == 4 && SART_ORIGIN_HEAD % SART_ORIGIN_CELL == 0, "a ray's three atomics fall into one aligned 32-byte cell");

// ------------------------------------------------------------------------------------------------
// aperture map of the histogram trace (include/sart.h: sart_trace_histogram_aperture_device)
// ------------------------------------------------------------------------------------------------
// The fourth user of the pipeline: the origin map's three atomics per passed ray, into the cell of a grid over the entrance plane that
// the ray's entrance point (X0, Y0 of ring 1: pointEntranceXRT, raytracer.nim:2091-2094) falls in - or into the one cell behind the
// grid, "outside the window".  The cell index is formed at the head of the phase-B pass, so that one 32-bit register and not the two
// doubles lives across phase B.  The head, its per-wave table, the partials and the fold are the origin map's.
struct ApertureKernArgs {
  HotA H;
  const DevBlob* blob;
  TraceArgs A;
  double* acc;
  HotB HB;
  ApertureArgs AP;
};
static_assert(offsetof(ApertureKernArgs, A) == offsetof(HistKernArgs, A) && offsetof(ApertureKernArgs, HB) == offsetof(HistKernArgs, HB) &&
                  offsetof(ApertureKernArgs, AP) == offsetof(HistKernArgs, SC),
              "the aperture kernel shares the argument offsets of the histogram kernel");
static_assert(SART_APERTURE_CELL == SART_ORIGIN_CELL && SART_APERTURE_HEAD == SART_ORIGIN_HEAD && SART_APERTURE_N == SART_ORIGIN_N &&
                  SART_APERTURE_SUM_WEIGHTS == SART_ORIGIN_SUM_WEIGHTS && SART_APERTURE_SUM_WEIGHTS_SQ == SART_ORIGIN_SUM_WEIGHTS_SQ &&
                  SART_APERTURE_N_PASSED == SART_ORIGIN_N_PASSED && SART_APERTURE_SUM_WEIGHTS_HI == SART_ORIGIN_SUM_WEIGHTS_HI &&
                  SART_APERTURE_SUM_WEIGHTS_SQ_HI == SART_ORIGIN_SUM_WEIGHTS_SQ_HI,
              "the aperture block is folded and finalized by the origin block's kernels");

// ------------------------------------------------------------------------------------------------
// the one pipeline of the four breakdowns: breakdown_histogram_body
// ------------------------------------------------------------------------------------------------
// What a breakdown is to the body: its kind, its argument struct and where the kernel arguments hold it, its per-workgroup table in
// LDS (in the last kTableCells cells behind the tables, the image tile's extra cells in front of it) and the slots it stores of it
// per workgroup.  What the breakdown does to a ray stands in the body itself, under `if constexpr (kShells / kChannels / kOrigin / kAperture)`:
// one ray can be followed through one function.
enum class BreakdownKind { Shells, Channels, Origin, Aperture };
struct ShellBreakdown {
  static constexpr BreakdownKind kKind = BreakdownKind::Shells;
  using Args = ShellArgs;
  static constexpr size_t kArgsOffset = offsetof(ShellKernArgs, SH);
  static constexpr int kTableCells = kShellTableCells;
  template <class Sum>
  struct Table {
    uint32_t cnt[kMaxShells][4];   // per shell: N_SELECTED, N_HIT_NICKEL, N_PASSED_TILL_WINDOW, N_PASSED
    Sum sum[kMaxShells][2];        // per shell: sum of w, sum of w^2
  };
};
struct ChannelBreakdown {
  static constexpr BreakdownKind kKind = BreakdownKind::Channels;
  using Args = ChannelArgs;
  static constexpr size_t kArgsOffset = offsetof(ChanKernArgs, CH);
  static constexpr int kTableCells = kChanTableCells;
  template <class Sum>
  struct Table {
    Sum sum[kMaxChannels][3][kChanLanes];     // per channel: sum of c, sum of c^2, sum of c outside the image
    uint32_t cnt[kMaxChannels][kChanLanes];   // per channel: N_CONTRIBUTING
  };
};
struct OriginBreakdown {
  static constexpr BreakdownKind kKind = BreakdownKind::Origin;
  using Args = OriginArgs;
  static constexpr size_t kArgsOffset = offsetof(OriginKernArgs, OG);
  static constexpr int kTableCells = kOriginTableCells;
  template <class Sum>
  struct Table {
    Sum head[kOriginTableCells / kOriginPartialSlots][kOriginPartialSlots];   // per wave: N_PASSED, sum of w, sum of w^2, unused
  };
};
struct ApertureBreakdown {
  static constexpr BreakdownKind kKind = BreakdownKind::Aperture;
  using Args = ApertureArgs;
  static constexpr size_t kArgsOffset = offsetof(ApertureKernArgs, AP);
  static constexpr int kTableCells = kApertureTableCells;
  template <class Sum>
  using Table = OriginBreakdown::Table<Sum>;   // one head row per wave, as the origin map's
};

template <int BLOCK, bool ROT, bool FIXED, class BD>
__device__ __forceinline__ void breakdown_histogram_body(HotA H, const DevBlob* __restrict__ blob, TraceArgs A, double* __restrict__ acc,
                                                         typename BD::Args BDarg) {
  using Sum = std::conditional_t<FIXED, long long, double>;   // per-lane sums: quanta (FIXED) or f64
  constexpr bool kShells = BD::kKind == BreakdownKind::Shells, kChannels = BD::kKind == BreakdownKind::Channels,
                 kOrigin = BD::kKind == BreakdownKind::Origin, kAperture = BD::kKind == BreakdownKind::Aperture;
  constexpr bool kHead = kOrigin || kAperture;   // the table is the head's rows, one per wave
  static_assert(!kHead || BLOCK / 64 == kOriginTableCells / kOriginPartialSlots, "one row of the origin table per wave");
  struct LdsLayout {
    TablesLds S;
    double tile_extra[kRingExtraCells - BD::kTableCells];   // cells kTileRingCells .. of the image tile
    typename BD::template Table<Sum> tab;
    DevBlob B;
    TraceArgs Ab;
    QueueLds<BLOCK / 64> Q;
  };
  __shared__ LdsLayout lds;
  TablesLds& S = lds.S;
  QueueLds<BLOCK / 64>& Q = lds.Q;
  static_assert((offsetof(LdsLayout, Q) % 512) == 0, "the rings are addressed with ds_*2st64 offsets");
  static_assert((BLOCK / 64) * kQueue == kTileRingCells, "ring 0 of this workgroup is the first part of the tile space");
  static_assert(sizeof(lds.tab) == BD::kTableCells * sizeof(double), "the breakdown table's cells");
  // cell t of the LDS image tile: ring 0 (stage A0 off: ray + u3hi columns, 128 doubles per wave), then the cells behind the tables
  auto tile_cell = [&](uint32_t t) -> double* {
    return t < (uint32_t)kTileRingCells ? reinterpret_cast<double*>(&Q.w[t >> 7].ray[0]) + (t & 127u)
                                        : &lds.tile_extra[t - (uint32_t)kTileRingCells];
  };
  DevBlob& B = lds.B;
  TraceArgs& Ab = lds.Ab;
  {
    const uint64_t* src = reinterpret_cast<const uint64_t*>(blob);
    uint64_t* dst = reinterpret_cast<uint64_t*>(&B);
    for (int i = threadIdx.x; i < (int)(sizeof(DevBlob) / 8); i += BLOCK) dst[i] = src[i];
    if (threadIdx.x == 0) Ab = A;
    __syncthreads();
  }
  const DevParams& Pb = B.P;
  const DevTables& Tb = B.T;
  {
    uint64_t* q = reinterpret_cast<uint64_t*>(&Q);
    for (int i = threadIdx.x; i < (int)(sizeof(Q) / 8); i += BLOCK) q[i] = 0ull;
    for (int i = threadIdx.x; i < kRingExtraCells - BD::kTableCells; i += BLOCK) lds.tile_extra[i] = 0.0;
    if constexpr (kShells) {
      for (int i = threadIdx.x; i < kMaxShells * 4; i += BLOCK) lds.tab.cnt[i >> 2][i & 3] = 0u;
      for (int i = threadIdx.x; i < kMaxShells * 2; i += BLOCK) lds.tab.sum[i >> 1][i & 1] = 0;
    } else if constexpr (kChannels) {
      for (int i = threadIdx.x; i < kMaxChannels * 3 * kChanLanes; i += BLOCK) (&lds.tab.sum[0][0][0])[i] = 0;
      if (threadIdx.x < kMaxChannels * kChanLanes) (&lds.tab.cnt[0][0])[threadIdx.x] = 0u;
    }   // (origin, aperture: every wave writes its whole row in the epilogue)
  }
  stage_tables<BLOCK>(S, Pb, Tb);   // (its barrier orders the zeroing above before the first use)
  const LdsTables L{S.sincos, S.rcdf_hi, Tb.flux_radius_cdf, S.rguide, S.shells, S.lut};

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint64_t waves_total = (uint64_t)gridDim.x * (BLOCK / 64);
  const uint64_t wave_global = (uint64_t)blockIdx.x * (BLOCK / 64) + wave;
  const bool early_reject = H.n_zones > 0;   // wave-uniform; the host builds no zones for the X-ray test source
  const uint64_t first_chunk = A.ray_id_offset >> 8;
  uint64_t id_base = first_chunk << 8;
  asm volatile("" : "+s"(id_base));
  const uint32_t rel_begin = (uint32_t)(A.ray_id_offset & 255u);
  const uint32_t rel_end = rel_begin + (uint32_t)A.n_rays;
  const uint32_t n_chunks = (rel_end + 255u) >> 8;

  uint32_t n_reached = 0, n_shell = 0, n_nickel = 0, n_till = 0, n_passed = 0;   // wave-uniform
  uint32_t n_outside = 0;    // per lane: passed rays outside the image
  Sum sum_w = 0, sum_w2 = 0, sum_x = 0, sum_y = 0, sum_r = 0;
  long long sum_wo = 0;      // FIXED: weights of the passed rays outside the image
  uint32_t h0 = 0, t0 = 0;   // ring 0 (A0 -> A1)
  uint32_t h1 = 0, t1 = 0;   // ring 1 (A1 -> B)
  auto ring_sync = [] {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  auto prefix_of = [](uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
  };
  [[maybe_unused]] auto shell_of = [](int shell) { return min((uint32_t)shell, (uint32_t)(kMaxShells - 1)); };   // (phase A: shell < n_shells <= 64)

  // phase A as in trace_histogram_kernel's generic variants.  Shells: every selected ray counts for its shell, those that the
  // shell0_miss_radius compare ends here included (their shell is shell 0)
  auto run_phase_a = [&](uint32_t rel, bool valid, uint32_t u3_hi) {
    SART_STAGE_MARK("A1");
    __builtin_amdgcn_s_setprio(SART_PRIO_A1);
    RayState st;
    bool sampled = false, reached = false;
    double radial;
    HotA Hl;
    reload_hot(Hl);
    LaneMasks M;
    (void)phase_a<false, ROT ? 1 : 0, false, false>(Hl, Pb, L, A.seed_lo, A.seed_hi, id_base + (uint64_t)rel, u3_hi, st, sampled, reached, radial, M);
    const uint64_t valid_m = ballot64(valid);
    n_reached += (uint32_t)__popcll(valid_m & M.reached);
    const uint64_t selected = valid_m & M.ok;
    n_shell += (uint32_t)__popcll(selected);
    if constexpr (kShells) {
      if (__builtin_amdgcn_inverse_ballot_w64(selected))
        __hip_atomic_fetch_add(&lds.tab.cnt[shell_of(st.shell)][0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    const uint64_t mask = selected & ~ballot64(radial < Pb.shell0_miss_radius);
    const uint32_t cnt = (uint32_t)__popcll(mask);
    if (__builtin_amdgcn_inverse_ballot_w64(mask)) {
      const uint32_t slot = (t1 + prefix_of(mask)) % kQueue;
      Q.w[wave].X0[slot] = st.X0; Q.w[wave].Y0[slot] = st.Y0;
      Q.w[wave].tsx[slot] = st.tsx; Q.w[wave].tsy[slot] = st.tsy;
      Q.w[wave].path[slot] = st.path_cb;
      Q.w[wave].u5[slot] = st.u5;
      Q.w[wave].idx[slot] = st.r_idx | (st.shell << 16);
    }
    t1 += cnt;
    __builtin_amdgcn_s_setprio(0);
  };

  auto run_phase_b = [&](uint32_t n_valid) {
    SART_STAGE_MARK("B");
    __builtin_amdgcn_s_setprio(SART_PRIO_B);
    RayState st;
    const bool valid = (uint32_t)lane < n_valid;
    const uint32_t slot = (h1 + (uint32_t)lane) % kQueue;
    RayOut out;
    [[maybe_unused]] uint32_t ap_cell = 0u;   // aperture: the entrance point's cell, nx ny where it lies outside the window
    {
      st.X0 = Q.w[wave].X0[slot]; st.Y0 = Q.w[wave].Y0[slot];
      st.tsx = Q.w[wave].tsx[slot]; st.tsy = Q.w[wave].tsy[slot];
      st.path_cb = Q.w[wave].path[slot];
      st.u5 = Q.w[wave].u5[slot];
      st.u5_hi = upper32_of_uniform(st.u5);   // u5 = word / 2^32 (uniforms_of): the word back, exactly
      if (!ROT) {
        st.zcb = -(H.dz3 - H.dz1);
      } else {
        st.zcb = zcb_rotated(Pb.rx_s, -Pb.rx_c * Pb.ry_s, Pb.rx_c * Pb.ry_c, Pb.half_length_telescope, st.X0 + Pb.entrance_x,
                             st.Y0 + Pb.entrance_y, st.tsx, st.tsy, H.dz3 - H.dz1);
      }
      const int packed = Q.w[wave].idx[slot];
      st.r_idx = packed & 0xFFFF;
      st.shell = packed >> 16;
      if constexpr (kAperture) {
        // binned as the image is (prepareHeatmap's rule): inside <=> 0 <= f < n on both axes, so a NaN falls outside.  Formed here,
        // from the ring's words, so that one 32-bit register lives across phase B.  nx ny <= kApertureMaxCells (host).
        typename BD::Args APl;
        reload_kernarg(APl, BD::kArgsOffset);
        const double fx = (st.X0 - APl.x_min) * APl.inv_step_x;
        const double fy = (st.Y0 - APl.y_min) * APl.inv_step_y;
        const bool in_window = (fx >= 0.0) & (fx < (double)APl.nx) & (fy >= 0.0) & (fy < (double)APl.ny);
        ap_cell = in_window ? (uint32_t)(int)fy * (uint32_t)APl.nx + (uint32_t)(int)fx : (uint32_t)APl.nx * (uint32_t)APl.ny;
      }
      const DevBlob& Bo = lds_opaque(B);
      HotB HB;
      reload_kernarg(HB, offsetof(HistKernArgs, HB));
      asm volatile("" :: "s"(HB.cdf_hi32), "s"(HB.energy_guide), "s"(HB.energy_records), "s"(HB.records_on), "s"(HB.energy_tab), "s"(HB.refl), "s"(HB.refl_n_angles), "s"(HB.cdf_stride));
      phase_b<false, false, -1, false>(Bo.P, L, HB, lds_opaque(Ab), st, H.test_active ? Pb.n_energies : -1, valid, out, nullptr);
    }
    h1 += n_valid;
    __builtin_amdgcn_s_setprio(SART_PRIO_ACC);
    n_nickel += (uint32_t)__popcll(out.m_nickel);
    n_till += (uint32_t)__popcll(out.m_till);
    n_passed += (uint32_t)__popcll(out.m_passed);
    [[maybe_unused]] const uint32_t sh = shell_of(st.shell);   // (shells)
    if constexpr (kShells) {
      if (__builtin_amdgcn_inverse_ballot_w64(out.m_nickel))
        __hip_atomic_fetch_add(&lds.tab.cnt[sh][1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (__builtin_amdgcn_inverse_ballot_w64(out.m_till))
        __hip_atomic_fetch_add(&lds.tab.cnt[sh][2], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    if (out.passed) {
      SART_STAGE_MARK("ACC");
      [[maybe_unused]] typename BD::Args BDl;     // (shells: re-read in the spectra branch)
      [[maybe_unused]] double f[kMaxChannels];    // channels: this ray's fractions
      [[maybe_unused]] uint32_t f_off = 0u;
      if constexpr (kChannels) {
        // this ray's fractions: requested first, used behind the accumulator's own work.  The indices are clamped to the table (host:
        // its shape is the solar tables' and it is < 4 GB, so the byte offset is 32-bit).
        reload_kernarg(BDl, BD::kArgsOffset);
        asm volatile("" :: "s"(BDl.block), "s"(BDl.frac), "s"(BDl.n_channels), "s"(BDl.stride), "s"(BDl.n_radii), "s"(BDl.n_energies),
                     "s"(BDl.n_energies1));
        // (the first half of the run here, the second - strides of 8 only: the same 64-byte line, a cache hit by then - in front of the
        // channel loop, where the first four channels' work covers it: all eight in flight across the accumulator's work spill registers)
        f_off = ((uint32_t)min(max(st.r_idx, 0), BDl.n_radii - 1) * (uint32_t)BDl.n_energies +
                 (uint32_t)min(max(out.e_idx, 0), BDl.n_energies - 1)) * ((uint32_t)BDl.stride * 8u);
#pragma unroll
        for (int k = 0; k < kMaxChannels; ++k) f[k] = 0.0;
        if (BDl.stride == 1) {   // wave-uniform
          f[0] = gload<double>(BDl.frac, f_off);
        } else {
#pragma unroll
          for (int k = 0; k < kMaxChannels / 4; ++k)
            if (2 * k < BDl.stride) {
              const d2 v = gload<d2>(BDl.frac, f_off + 16u * (uint32_t)k);
              f[2 * k] = v.x;
              f[2 * k + 1] = v.y;
            }
        }
      }
      TraceArgs Al;
      reload_kernarg(Al, offsetof(HistKernArgs, A));
      asm volatile("" :: "s"(Al.replicas), "s"(Al.replica_mask), "s"(Al.replica_stride), "s"(Al.image_nx), "s"(Al.image_ny),
                   "s"(Al.image_x_min), "s"(Al.image_y_min), "s"(Al.image_inv_step_x), "s"(Al.image_inv_step_y), "s"(Al.spectra),
                   "s"(Al.tile_x0), "s"(Al.tile_y0), "s"(Al.tile_n), "s"(Al.tile_base));
      if constexpr (kShells) __hip_atomic_fetch_add(&lds.tab.cnt[sh][3], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      long long w_fx = 0;   // FIXED: this ray's weight in quanta (what the image, the sums and the spectra add)
      [[maybe_unused]] long long w2_fx = 0;   //        and its squared weight's (what SUM_WEIGHTS_SQ adds; origin: and the ray's cell)
      if constexpr (FIXED) {
        w_fx = to_fixed(out.weight, Al.fx_scale_w);
        w2_fx = to_fixed(out.weight * out.weight, Al.fx_scale_w2);
        sum_w += w_fx;
        sum_w2 += w2_fx;
        sum_x += to_fixed(out.px, kFixedPositionScale);
        sum_y += to_fixed(out.py, kFixedPositionScale);
        sum_r += to_fixed(out.rdet, kFixedPositionScale);
        if constexpr (kShells) {
          // the same integers the scalars add: the per-shell sums add up to SUM_WEIGHTS / SUM_WEIGHTS_SQ exactly
          __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(&lds.tab.sum[sh][0]), (unsigned long long)w_fx, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_WORKGROUP);
          __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(&lds.tab.sum[sh][1]), (unsigned long long)w2_fx, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      } else {
        sum_w += out.weight;
        sum_w2 = fma(out.weight, out.weight, sum_w2);
        sum_x += out.px;
        sum_y += out.py;
        sum_r += out.rdet;
        if constexpr (kShells) {
          __hip_atomic_fetch_add(&lds.tab.sum[sh][0], out.weight, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          __hip_atomic_fetch_add(&lds.tab.sum[sh][1], out.weight * out.weight, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
      // prepareHeatmap (:838-842), as trace_histogram_kernel bins it
      const double fx = (out.px - Al.image_x_min) * Al.image_inv_step_x;
      const double fy = (out.py - Al.image_y_min) * Al.image_inv_step_y;
      const int nx = Al.image_nx, ny = Al.image_ny;
      const uint64_t inside_m = ballot64(fx >= 0.0) & ballot64(fx < (double)nx) & ballot64(fy >= 0.0) & ballot64(fy < (double)ny);
      const bool inside = __builtin_amdgcn_inverse_ballot_w64(inside_m);
      n_outside += inside ? 0u : 1u;
      if constexpr (FIXED) {
        if (out.m_passed & ~inside_m) sum_wo += inside ? 0ll : w_fx;
      }
      double* const img = Al.replicas + (size_t)((uint32_t)wave_global & Al.replica_mask) * (size_t)Al.replica_stride;
      [[maybe_unused]] uint32_t c_pix = 0u;   // the ray's pixel, for the channel images
      if (inside) {
        const uint32_t ix = (uint32_t)(int)fx, iy = (uint32_t)(int)fy;
        if constexpr (kChannels) c_pix = iy * (uint32_t)nx + ix;
        const uint32_t tn = (uint32_t)Al.tile_n;
        const uint32_t tx = ix - (uint32_t)Al.tile_x0, ty = iy - (uint32_t)Al.tile_y0;
        if ((tx < tn) & (ty < tn)) {
          const uint32_t t = ty * tn + tx + (uint32_t)Al.tile_base;   // < kTileRingCells + kRingExtraCells - BD::kTableCells (host)
          if constexpr (FIXED)
            __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(tile_cell(t)), (unsigned long long)w_fx, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_WORKGROUP);
          else
            __hip_atomic_fetch_add(tile_cell(t), out.weight, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
          const uint32_t pix = iy * (uint32_t)nx + ix;
          typedef __attribute__((address_space(1))) char* gbytes;
          if constexpr (FIXED) atomic_add_slot_i64((double*)((gbytes)img + pix * 8u), w_fx);
          else unsafeAtomicAdd((double*)((gbytes)img + pix * 8u), out.weight);
        }
      }
      if (Al.spectra) {   // wave-uniform: the spectra behind the scalars; shells: and the same energy bins per shell in the block
        double* rad = acc + (size_t)nx * (size_t)ny + SART_ACC_COUNT;
        double* en = rad + 2 * (size_t)Al.n_radial_bins;
        const size_t ne1 = (size_t)Pb.n_energies + 1;
        const int rb = min((int)(out.rdet * Al.radial_inv_bin), Al.n_radial_bins - 1);
        [[maybe_unused]] double* sen = nullptr;   // shells: counts[sh][e]
        [[maybe_unused]] size_t sw_off = 0;       //         -> weights[sh][e]
        if constexpr (kShells) {
          reload_kernarg(BDl, BD::kArgsOffset);
          sen = BDl.block + (size_t)BDl.n_shells * SART_SHELL_ROW + (size_t)sh * ne1 + (size_t)out.e_idx;
          sw_off = (size_t)BDl.n_shells * ne1;
        }
        if constexpr (FIXED) {
          atomic_add_slot_i64(&rad[rb], 1);
          atomic_add_slot_i64(&rad[(size_t)Al.n_radial_bins + rb], w_fx);
          atomic_add_slot_i64(&en[out.e_idx], 1);
          atomic_add_slot_i64(&en[ne1 + out.e_idx], w_fx);
          atomic_add_slot_i64(&en[2 * ne1 + out.e_idx], to_fixed(out.reflect, kFixedReflectScale));
          if constexpr (kShells) {
            atomic_add_slot_i64(sen, 1);
            atomic_add_slot_i64(sen + sw_off, w_fx);
          }
        } else {
          unsafeAtomicAdd(&rad[rb], 1.0);
          unsafeAtomicAdd(&rad[(size_t)Al.n_radial_bins + rb], out.weight);
          unsafeAtomicAdd(&en[out.e_idx], 1.0);
          unsafeAtomicAdd(&en[ne1 + out.e_idx], out.weight);
          unsafeAtomicAdd(&en[2 * ne1 + out.e_idx], out.reflect);
          if constexpr (kShells) {
            unsafeAtomicAdd(sen, 1.0);
            unsafeAtomicAdd(sen + sw_off, out.weight);
          }
        }
      }
      // the origin map: the ray's cell (r_idx, e_idx) takes 1, w and w^2 - FIXED: the integers the scalars add, so the cells add up to
      // the head exactly -, three atomics into one aligned 32-byte cell behind the accumulator's own.  The indices are clamped to the
      // map (host: its shape is the solar tables').
      if constexpr (kOrigin) {
        reload_kernarg(BDl, BD::kArgsOffset);
        const size_t cell = (size_t)min(max(st.r_idx, 0), BDl.n_radii - 1) * (size_t)BDl.n_energies +
                            (size_t)min(max(out.e_idx, 0), BDl.n_energies - 1);
        double* const oc = BDl.block + SART_ORIGIN_HEAD + cell * SART_ORIGIN_CELL;
        if constexpr (FIXED) {
          atomic_add_slot_i64(oc + SART_ORIGIN_N, 1);
          atomic_add_slot_i64(oc + SART_ORIGIN_SUM_WEIGHTS, w_fx);
          atomic_add_slot_i64(oc + SART_ORIGIN_SUM_WEIGHTS_SQ, w2_fx);
        } else {
          unsafeAtomicAdd(oc + SART_ORIGIN_N, 1.0);
          unsafeAtomicAdd(oc + SART_ORIGIN_SUM_WEIGHTS, out.weight);
          unsafeAtomicAdd(oc + SART_ORIGIN_SUM_WEIGHTS_SQ, out.weight * out.weight);
        }
      }
      // the aperture map: the cell of the ray's entrance point (or the outside cell) takes the same 1, w and w^2, in the same way
      if constexpr (kAperture) {
        reload_kernarg(BDl, BD::kArgsOffset);
        double* const ac = BDl.block + SART_APERTURE_HEAD + (size_t)ap_cell * SART_APERTURE_CELL;
        if constexpr (FIXED) {
          atomic_add_slot_i64(ac + SART_APERTURE_N, 1);
          atomic_add_slot_i64(ac + SART_APERTURE_SUM_WEIGHTS, w_fx);
          atomic_add_slot_i64(ac + SART_APERTURE_SUM_WEIGHTS_SQ, w2_fx);
        } else {
          unsafeAtomicAdd(ac + SART_APERTURE_N, 1.0);
          unsafeAtomicAdd(ac + SART_APERTURE_SUM_WEIGHTS, out.weight);
          unsafeAtomicAdd(ac + SART_APERTURE_SUM_WEIGHTS_SQ, out.weight * out.weight);
        }
      }
      // the channels: c_t = w f_t, ONE product; the same c_t to the row, the ray's energy bin and its pixel (or the row's OUTSIDE)
      if constexpr (kChannels) {
        const uint32_t cl = (uint32_t)lane & (uint32_t)(kChanLanes - 1);
        const size_t c_ne1 = (size_t)BDl.n_energies1, c_nimg = (size_t)nx * (size_t)ny;
        double* const c_en = BDl.block + (size_t)BDl.n_channels * SART_CHAN_ROW;                  // energy_weights[t][e]
        double* const c_img = c_en + (Al.spectra ? (size_t)BDl.n_channels * c_ne1 : (size_t)0);   // images [t][ny][nx]
        if (BDl.stride == 8) {   // wave-uniform: the second half of the run
#pragma unroll
          for (int k = kMaxChannels / 4; k < kMaxChannels / 2; ++k) {
            const d2 v = gload<d2>(BDl.frac, f_off + 16u * (uint32_t)k);
            f[2 * k] = v.x;
            f[2 * k + 1] = v.y;
          }
        }
#pragma unroll
        for (int t = 0; t < kMaxChannels; ++t) {
          if (t >= BDl.n_channels) break;   // wave-uniform
          const double ft = f[t];
          if (ft > 0.0) __hip_atomic_fetch_add(&lds.tab.cnt[t][cl], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          const double c = out.weight * ft;
          if (c != 0.0) {
            if constexpr (FIXED) {
              const long long c_fx = to_fixed(c, Al.fx_scale_w);
              const long long c2_fx = to_fixed(c * c, Al.fx_scale_w2);
              __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(&lds.tab.sum[t][0][cl]), (unsigned long long)c_fx,
                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(&lds.tab.sum[t][1][cl]), (unsigned long long)c2_fx,
                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              if (inside) atomic_add_slot_i64(c_img + (size_t)t * c_nimg + c_pix, c_fx);
              else
                __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(&lds.tab.sum[t][2][cl]), (unsigned long long)c_fx,
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              if (Al.spectra) atomic_add_slot_i64(c_en + (size_t)t * c_ne1 + (size_t)out.e_idx, c_fx);
            } else {
              __hip_atomic_fetch_add(&lds.tab.sum[t][0][cl], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              __hip_atomic_fetch_add(&lds.tab.sum[t][1][cl], c * c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              if (inside) unsafeAtomicAdd(c_img + (size_t)t * c_nimg + c_pix, c);
              else __hip_atomic_fetch_add(&lds.tab.sum[t][2][cl], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              if (Al.spectra) unsafeAtomicAdd(c_en + (size_t)t * c_ne1 + (size_t)out.e_idx, c);
            }
          }
        }
      }
    }
    __builtin_amdgcn_s_setprio(0);
  };

  // stage A0 as in the generic histogram variants (zone bounds re-read from the kernel arguments per pass)
  uint32_t chunk = (uint32_t)wave_global;
  const uint32_t lane4 = 4u * (uint32_t)lane;
  uint32_t pass = 0;
  U4 stream = U4{0u, 0u, 0u, 0u};
  for (;;) {
    const bool have_new = chunk < n_chunks;   // wave-uniform
    SART_STAGE_MARK("LOOP");
    if (have_new) {
      SART_STAGE_MARK("A0");
      if (pass == 0u) stream = stream_block(((first_chunk + (uint64_t)chunk) << 6) + (uint64_t)lane, A.seed_lo, A.seed_hi);
      const uint32_t w = word_of(stream, pass);
      const uint32_t rel = ((chunk << 8) + pass) + lane4;
      if (early_reject) {
        ZoneTable Z;
        reload_zones(Z);
        uint64_t dead_m = 0, reached_m = 0;
#pragma unroll
        for (int z = 0; z < kMaxZones; ++z) {
          const uint64_t in = ballot64(w >= Z.lo[z]) & ballot64(w <= Z.hi[z]);
          dead_m |= in;
          reached_m |= ((Z.zone_reached >> z) & 1u) ? in : 0ull;
        }
        const uint32_t chunk_lo = chunk << 8;
        uint64_t valid_m = ~0ull;
        if ((chunk_lo < rel_begin) | (chunk_lo + 256u > rel_end)) valid_m = ballot64(rel >= rel_begin) & ballot64(rel < rel_end);
        n_reached += (uint32_t)__popcll(valid_m & reached_m);
        const uint64_t mask = valid_m & ~dead_m;
        if (__builtin_amdgcn_inverse_ballot_w64(mask)) {
          const uint32_t slot = (t0 + prefix_of(mask)) % kQueue;
          Q.w[wave].ray[slot] = rel;
          Q.w[wave].u3hi[slot] = w;
        }
        t0 += (uint32_t)__popcll(mask);
      } else {
        run_phase_a(rel, (rel >= rel_begin) & (rel < rel_end), w);
      }
      pass = (pass + 1u) & 3u;
      if (pass == 0u) chunk += (uint32_t)waves_total;
      ring_sync();
    }
    if (early_reject) {
      const uint32_t n0 = t0 - h0;
      if ((n0 >= 64u) | (!have_new & (n0 > 0u))) {
        const uint32_t m = min(n0, 64u);
        const bool v = (uint32_t)lane < m;
        const uint32_t slot = (h0 + (uint32_t)lane) % kQueue;
        const uint32_t rel = Q.w[wave].ray[slot];
        const uint32_t w = Q.w[wave].u3hi[slot];
        h0 += m;
        run_phase_a(rel, v, w);
        ring_sync();
      }
    }
    const uint32_t n1 = t1 - h1;
    const bool draining = !have_new & (t0 == h0);
    if ((n1 >= 64u) | (draining & (n1 > 0u))) {
      run_phase_b(min(n1, 64u));
      ring_sync();
    }
    if (draining & (t1 == h1)) break;
  }

  SART_STAGE_MARK("EPILOGUE");
  // flush of the LDS image tile: one global atomic per non-empty tile pixel and workgroup
  if (A.tile_n > 0) {
    __syncthreads();
    const uint32_t tn = (uint32_t)A.tile_n, n_tile = tn * tn;
    double* const img = A.replicas + (size_t)((uint32_t)wave_global & A.replica_mask) * (size_t)A.replica_stride;
    for (uint32_t t = threadIdx.x; t < n_tile; t += BLOCK) {
      const double v = *tile_cell(t + (uint32_t)A.tile_base);
      if (__double_as_longlong(v) != 0ll) {
        const uint32_t ty = t / tn, tx = t - ty * tn;
        double* const px = &img[(size_t)((uint32_t)A.tile_y0 + ty) * (size_t)A.image_nx + ((uint32_t)A.tile_x0 + tx)];
        if constexpr (FIXED) atomic_add_slot_i64(px, __double_as_longlong(v));
        else unsafeAtomicAdd(px, v);
      }
    }
  }
  // scalars: as trace_histogram_kernel (wave reduction -> LDS staging in wave 0's first ring columns -> one store per workgroup)
  __syncthreads();
  Sum (*const red)[SART_ACC_COUNT] = reinterpret_cast<Sum (*)[SART_ACC_COUNT]>(&Q.w[0].X0[0]);
  Sum sw, sw2, sxx, syy, srr;
  if constexpr (FIXED) {
    sw = wave_sum_i64(sum_w); sw2 = wave_sum_i64(sum_w2); sxx = wave_sum_i64(sum_x); syy = wave_sum_i64(sum_y); srr = wave_sum_i64(sum_r);
  } else {
    sw = wave_sum(sum_w); sw2 = wave_sum(sum_w2); sxx = wave_sum(sum_x); syy = wave_sum(sum_y); srr = wave_sum(sum_r);
  }
  const long long swo = FIXED ? wave_sum_i64(sum_wo) : 0ll;
  const long long n_out = wave_sum_i64((long long)n_outside);
  if (lane == 0) {
    Sum* r = red[wave];
    for (int k = 0; k < SART_ACC_COUNT; ++k) r[k] = 0;
    r[SART_ACC_SUM_WEIGHTS] = sw;
    r[SART_ACC_SUM_WEIGHTS_SQ] = sw2;
    r[SART_ACC_SUM_X] = sxx;
    r[SART_ACC_SUM_Y] = syy;
    r[SART_ACC_SUM_R] = srr;
    r[SART_ACC_N_PASSED] = (Sum)n_passed;
    r[SART_ACC_N_PASSED_TILL_WINDOW] = (Sum)n_till;
    r[SART_ACC_N_HIT_NICKEL] = (Sum)n_nickel;
    r[SART_ACC_N_REACHED_TELESCOPE] = (Sum)n_reached;
    r[SART_ACC_N_SHELL_SELECTED] = (Sum)n_shell;
    r[SART_ACC_N_OUTSIDE_IMAGE] = (Sum)n_out;
    if constexpr (FIXED) r[SART_ACC_SUM_WEIGHTS_OUTSIDE] = swo;
    if constexpr (kHead) {   // the head's row of this wave: the very sums the scalars take
      lds.tab.head[wave][0] = (Sum)n_passed;
      lds.tab.head[wave][1] = sw;
      lds.tab.head[wave][2] = sw2;
      lds.tab.head[wave][3] = 0;
    }
  }
  __syncthreads();
  if (threadIdx.x < SART_ACC_COUNT) {
    Sum t = 0;
    for (int w = 0; w < BLOCK / 64; ++w) t += red[w][threadIdx.x];
    reinterpret_cast<Sum*>(A.partials)[(size_t)blockIdx.x * SART_ACC_COUNT + threadIdx.x] = t;
  }
  // the breakdown table of this workgroup (every wave has left the loop: the barriers above)
  if constexpr (kHead) {
    if (threadIdx.x < kOriginPartialSlots) {
      Sum t = 0;
      for (int w = 0; w < BLOCK / 64; ++w) t += lds.tab.head[w][threadIdx.x];
      reinterpret_cast<Sum*>(BDarg.partials)[(size_t)blockIdx.x * kOriginPartialSlots + threadIdx.x] = t;
    }
  } else if constexpr (kShells) {
    for (int i = threadIdx.x; i < kMaxShells * kShellPartialSlots; i += BLOCK) {
      const int s = i / kShellPartialSlots, j = i - s * kShellPartialSlots;
      const Sum v = j < 4 ? (Sum)lds.tab.cnt[s][j] : lds.tab.sum[s][j - 4];
      reinterpret_cast<Sum*>(BDarg.partials)[(size_t)blockIdx.x * (kMaxShells * kShellPartialSlots) + i] = v;
    }
  } else if (threadIdx.x < kMaxChannels * kChanPartialSlots) {
    const int t = threadIdx.x / kChanPartialSlots, j = threadIdx.x - t * kChanPartialSlots;
    Sum v = 0;
    if (j < 3) {
      for (int l = 0; l < kChanLanes; ++l) v += lds.tab.sum[t][j][l];
    } else {
      uint32_t n = 0u;
      for (int l = 0; l < kChanLanes; ++l) n += lds.tab.cnt[t][l];
      v = (Sum)n;
    }
    reinterpret_cast<Sum*>(BDarg.partials)[(size_t)blockIdx.x * (kMaxChannels * kChanPartialSlots) + threadIdx.x] = v;
  }
}

// The four kernels: their names, template parameters and parameter lists are what the host launches and the code objects' tests know.
template <int BLOCK, bool ROT, bool FIXED>
__global__ __launch_bounds__(BLOCK) void shell_histogram_kernel(HotA H, const DevBlob* __restrict__ blob, TraceArgs A,
                                                                double* __restrict__ acc, HotB HBarg, ShellArgs SHarg) {
  breakdown_histogram_body<BLOCK, ROT, FIXED, ShellBreakdown>(H, blob, A, acc, SHarg);
}
template <int BLOCK, bool ROT, bool FIXED>
__global__ __launch_bounds__(BLOCK) void channel_histogram_kernel(HotA H, const DevBlob* __restrict__ blob, TraceArgs A,
                                                                  double* __restrict__ acc, HotB HBarg, ChannelArgs CHarg) {
  breakdown_histogram_body<BLOCK, ROT, FIXED, ChannelBreakdown>(H, blob, A, acc, CHarg);
}
template <int BLOCK, bool ROT, bool FIXED>
__global__ __launch_bounds__(BLOCK) void origin_histogram_kernel(HotA H, const DevBlob* __restrict__ blob, TraceArgs A,
                                                                 double* __restrict__ acc, HotB HBarg, OriginArgs OGarg) {
  breakdown_histogram_body<BLOCK, ROT, FIXED, OriginBreakdown>(H, blob, A, acc, OGarg);
}
template <int BLOCK, bool ROT, bool FIXED>
__global__ __launch_bounds__(BLOCK) void aperture_histogram_kernel(HotA H, const DevBlob* __restrict__ blob, TraceArgs A,
                                                                   double* __restrict__ acc, HotB HBarg, ApertureArgs AParg) {
  breakdown_histogram_body<BLOCK, ROT, FIXED, ApertureBreakdown>(H, blob, A, acc, AParg);
}

// ------------------------------------------------------------------------------------------------
// fused energy scan (include/sart.h: sart_trace_energy_scan)
// ------------------------------------------------------------------------------------------------
// With the X-ray test source (sart_setup_t::test_active) the energy is a constant of the setup (energyAx = testSource.energy,
// raytracer.nim:1771) and nothing geometric depends on it: it enters a ray through the reflectivities (:2126), the magnet
// transmission - conversion and absorption in gas (:1582-1625) -, the window / strongback transmission (:2170, :2179) and the
// gas absorption in the detector (:2190), all of them weight factors.  This kernel therefore runs phase A and the geometric part of
// phase B (mirrors, the reflection angles' cells and the fractions inside them, detector plane, chip, strips: phase_b<ESCAN>) ONCE
// per ray and then walks the launch's energies (wave-uniform; EScanArgs in the kernel arguments, read with scalar loads): gathers
// the two reflectivity pairs of energy k from the scan's own table (those of energy k + 1 are requested before the arithmetic of
// energy k), forms the weight with the arithmetic of the single launch in its order (the bitwise contract of the FIXED64 mode) and
// adds w, w^2 into per-energy LDS cells ([k][2][kScanLanes] in ring 0's space: the test source runs no stage A0) and the two
// energy-dependent counters N_PASSED, N_PASSED_TILL_WINDOW (weight != 0, :2135, :2220) into per-energy LDS counters; both are folded
// once per workgroup.  The energy-independent counters (N_REACHED_TELESCOPE, N_SHELL_SELECTED, N_HIT_NICKEL) go to the scalar
// partials of the histogram kernels.  Generic variants only (hist_variant_of 1 / 2: ROT), the stage read at run time.
struct EScanKernArgs {
  HotA H;
  const DevBlob* blob;
  TraceArgs A;
  double* unused;      // (keeps the argument offsets of trace_histogram_kernel: the reload_* helpers are shared)
  HotB HB;
  EScanArgs EN;
};
static_assert(offsetof(EScanKernArgs, A) == offsetof(HistKernArgs, A) && offsetof(EScanKernArgs, HB) == offsetof(HistKernArgs, HB) &&
                  offsetof(EScanKernArgs, EN) == offsetof(HistKernArgs, SC),
              "the energy-scan kernel shares the argument offsets of the histogram kernel");
static_assert(kEScanMaxEnergies * 2 * kScanLanes <= kTileRingCells, "the per-energy sums live in ring 0's 128 doubles per wave");

template <int BLOCK, bool ROT, bool FIXED>
__global__ __launch_bounds__(BLOCK) void energy_scan_kernel(HotA H, const DevBlob* __restrict__ blob, TraceArgs A,
                                                                  double* __restrict__ unused, HotB HBarg, EScanArgs ENarg) {
  struct LdsLayout {
    TablesLds S;
    DevBlob B;
    TraceArgs Ab;
    uint32_t cnt[kEScanMaxEnergies][2];   // per energy: N_PASSED, N_PASSED_TILL_WINDOW of this workgroup
    uint32_t shared_cnt[4];                // N_REACHED_TELESCOPE, N_SHELL_SELECTED, N_HIT_NICKEL of this workgroup
    alignas(512) QueueLds<BLOCK / 64> Q;
  };
  __shared__ LdsLayout lds;
  TablesLds& S = lds.S;
  QueueLds<BLOCK / 64>& Q = lds.Q;
  static_assert((offsetof(LdsLayout, Q) % 512) == 0, "the rings are addressed with ds_*2st64 offsets");
  static_assert(BLOCK == 1024, "[energy][2][32] cells fill ring 0 of 16 waves");
  // cell t of the per-energy sums: ring 0 (ray + u3hi columns, 128 doubles per wave), unused without stage A0
  auto cell = [&](uint32_t t) -> double* { return reinterpret_cast<double*>(&Q.w[t >> 7].ray[0]) + (t & 127u); };
  DevBlob& B = lds.B;
  TraceArgs& Ab = lds.Ab;
  {
    const uint64_t* src = reinterpret_cast<const uint64_t*>(blob);
    uint64_t* dst = reinterpret_cast<uint64_t*>(&B);
    for (int i = threadIdx.x; i < (int)(sizeof(DevBlob) / 8); i += BLOCK) dst[i] = src[i];
    if (threadIdx.x == 0) Ab = A;
    uint64_t* q = reinterpret_cast<uint64_t*>(&Q);
    for (int i = threadIdx.x; i < (int)(sizeof(Q) / 8); i += BLOCK) q[i] = 0ull;
    if (threadIdx.x < 2 * kEScanMaxEnergies) lds.cnt[threadIdx.x >> 1][threadIdx.x & 1] = 0u;
    if (threadIdx.x < 4) lds.shared_cnt[threadIdx.x] = 0u;
    __syncthreads();
  }
  const DevParams& Pb = B.P;
  const DevTables& Tb = B.T;
  stage_tables<BLOCK>(S, Pb, Tb);
  const LdsTables L{S.sincos, S.rcdf_hi, Tb.flux_radius_cdf, S.rguide, S.shells, S.lut};

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint64_t waves_total = (uint64_t)gridDim.x * (BLOCK / 64);
  const uint64_t wave_global = (uint64_t)blockIdx.x * (BLOCK / 64) + wave;
  const uint64_t first_chunk = A.ray_id_offset >> 8;
  uint64_t id_base = first_chunk << 8;
  asm volatile("" : "+s"(id_base));
  const uint32_t rel_begin = (uint32_t)(A.ray_id_offset & 255u);
  const uint32_t rel_end = rel_begin + (uint32_t)A.n_rays;
  const uint32_t n_chunks = (rel_end + 255u) >> 8;

  uint32_t n_reached = 0, n_shell = 0, n_nickel = 0;   // wave-uniform
  uint32_t h1 = 0, t1 = 0;   // ring 1 (A1 -> B)
  auto ring_sync = [] {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  auto prefix_of = [](uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
  };

  // phase A as in trace_histogram_kernel (generic variants: no stage A0, the path carried through ring 1)
  auto run_phase_a = [&](uint32_t rel, bool valid, uint32_t u3_hi) {
    SART_STAGE_MARK("A1");
    __builtin_amdgcn_s_setprio(SART_PRIO_A1);
    RayState st;
    bool sampled = false, reached = false;
    double radial;
    HotA Hl;
    reload_hot(Hl);
    LaneMasks M;
    (void)phase_a<false, ROT ? 1 : 0, false, false>(Hl, Pb, L, A.seed_lo, A.seed_hi, id_base + (uint64_t)rel, u3_hi, st, sampled, reached, radial, M);
    const uint64_t valid_m = ballot64(valid);
    n_reached += (uint32_t)__popcll(valid_m & M.reached);
    const uint64_t selected = valid_m & M.ok;
    n_shell += (uint32_t)__popcll(selected);
    const uint64_t mask = selected & ~ballot64(radial < Pb.shell0_miss_radius);
    const uint32_t cnt = (uint32_t)__popcll(mask);
    if (__builtin_amdgcn_inverse_ballot_w64(mask)) {
      const uint32_t slot = (t1 + prefix_of(mask)) % kQueue;
      Q.w[wave].X0[slot] = st.X0; Q.w[wave].Y0[slot] = st.Y0;
      Q.w[wave].tsx[slot] = st.tsx; Q.w[wave].tsy[slot] = st.tsy;
      Q.w[wave].path[slot] = st.path_cb;
      Q.w[wave].u5[slot] = st.u5;
      Q.w[wave].idx[slot] = st.r_idx | (st.shell << 16);
    }
    t1 += cnt;
    __builtin_amdgcn_s_setprio(0);
  };

  auto run_phase_b = [&](uint32_t n_valid) {
    SART_STAGE_MARK("B");
    __builtin_amdgcn_s_setprio(SART_PRIO_B);
    RayState st;
    const bool valid = (uint32_t)lane < n_valid;
    const uint32_t slot = (h1 + (uint32_t)lane) % kQueue;
    RayOut out;
    EScanGeo geo;
    st.X0 = Q.w[wave].X0[slot]; st.Y0 = Q.w[wave].Y0[slot];
    st.tsx = Q.w[wave].tsx[slot]; st.tsy = Q.w[wave].tsy[slot];
    st.path_cb = Q.w[wave].path[slot];
    st.u5 = Q.w[wave].u5[slot];
    if (!ROT) {
      st.zcb = -(H.dz3 - H.dz1);
    } else {
      st.zcb = zcb_rotated(Pb.rx_s, -Pb.rx_c * Pb.ry_s, Pb.rx_c * Pb.ry_c, Pb.half_length_telescope, st.X0 + Pb.entrance_x,
                           st.Y0 + Pb.entrance_y, st.tsx, st.tsy, H.dz3 - H.dz1);
    }
    const int packed = Q.w[wave].idx[slot];
    st.r_idx = packed & 0xFFFF;
    st.shell = packed >> 16;
    const DevBlob& Bo = lds_opaque(B);
    {
      HotB HB;
      reload_kernarg(HB, offsetof(EScanKernArgs, HB));
      phase_b<false, false, -1, false, false, true, true>(Bo.P, L, HB, lds_opaque(Ab), st, 0, valid, out, nullptr, &geo);
    }
    h1 += n_valid;
    n_nickel += (uint32_t)__popcll(out.m_nickel);
    if (!geo.m_live) { __builtin_amdgcn_s_setprio(0); return; }   // wave-uniform: no ray behind the mirrors, nothing counts

    SART_STAGE_MARK("ESCAN");
    asm volatile("; hot: per-energy loop of the fused energy scan");
    struct { int32_t n_energies, row_stride; const double* partials; const double* refl; } hdr;
    reload_kernarg(hdr, offsetof(EScanKernArgs, EN));
    const DevParams& P = Bo.P;
    const uint32_t flags = (uint32_t)__builtin_amdgcn_readfirstlane((int)Ab.flags);
    const int stage_gas = __builtin_amdgcn_readfirstlane(P.stage_gas);
    const int n_half_strips = __builtin_amdgcn_readfirstlane(P.n_half_strips);
    const int n_angles = __builtin_amdgcn_readfirstlane(P.refl_n_angles);
    const bool use_refl = !(flags & SART_CF_IGNORE_REFLECTION);
    const bool use_prob = !(flags & SART_CF_IGNORE_CONV_PROB);
    // the energy-independent factors, as phase_b forms them
    const double path_cb = geo.path_cb;
    double prob_vac = 1.0;
    if (!stage_gas && use_prob) prob_vac = P.conv_k * path_cb * path_cb;   // conversionProb (:363-365)
    const double path_len = path_cb;
    const double Lnat = path_len * P.gas_inv_hbarc_m;
    const double dist = geo.distance_pipe_m;
    const double term1 = P.gas_term1, dm2_abs = P.gas_dm2_abs;
    const GasCos cos_lead = GasCos::make();
    const bool strip = __builtin_amdgcn_inverse_ballot_w64(geo.m_strip);
    // refl[coating][row][angle] of the scan's table: 32-bit byte offsets (the table is < 4 GB, checked on the host)
    const uint32_t step = (uint32_t)n_angles * 8u;
    const uint32_t row0 = __umul24((uint32_t)(L.shells[st.shell].coating * hdr.row_stride), (uint32_t)n_angles);
    uint32_t off1 = (row0 + (uint32_t)geo.ia1) * 8u, off2 = (row0 + (uint32_t)geo.ia2) * 8u;
    d2 n1 = {1.0, 1.0}, n2 = {1.0, 1.0};
    if (use_refl) { n1 = gload<d2>(hdr.refl, off1); n2 = gload<d2>(hdr.refl, off2); }
    for (int k = 0; k < hdr.n_energies; ++k) {   // wave-uniform
      const d2 g1 = n1, g2 = n2;
      if (use_refl & (k + 1 < hdr.n_energies)) {   // energy k + 1's pairs in flight behind energy k's arithmetic
        off1 += step; off2 += step;
        n1 = gload<d2>(hdr.refl, off1);
        n2 = gload<d2>(hdr.refl, off2);
      }
      EScanEnergy E;
      reload_kernarg(E, offsetof(EScanKernArgs, EN) + offsetof(EScanArgs, e) + (size_t)k * sizeof(EScanEnergy));
      // ---- weights (:2116-2128), phase_b's arithmetic in its order ----
      double trans_magnet;
      GasRay gas = {0.0, 0.0, 0.0, 0.0, 0.0};
      if (!stage_gas) {
        trans_magnet = geo.cos_ya * prob_vac;   // (x absorb = 1: exact)
      } else {
        if (use_prob) {
          const double g = E.gamma;
          const double eh = exp_neg(-g * Lnat * 0.5);
          gas = GasRay{E.inv_two_e_ev, g * g * 0.25, -2.0 * eh, fma(eh, eh, 1.0), Lnat};
        }
        const double absorb = exp_neg(-fma(E.mu_pipe, dist, E.mu_magnet * (path_len * 1e-3)));
        trans_magnet = geo.cos_ya * absorb;
      }
      const double reflectv = fma(geo.xu1, g1.y - g1.x, g1.x) * fma(geo.xu2, g2.y - g2.x, g2.x);
      double w = reflectv * trans_magnet;
      uint64_t till_m = geo.m_live & ballot64(w != 0.0);
      const double trans_window = (n_half_strips > 0) ? (strip ? E.t_strongback : E.t_window) : 0.0;
      if (!(flags & SART_CF_IGNORE_DET_WINDOW)) { asm volatile(""); w *= trans_window; }
      if (!(flags & SART_CF_IGNORE_GAS_ABS)) { asm volatile(""); w *= E.a_gas; }
      if (!(flags & SART_CF_XRAY_TEST)) { asm volatile(""); w *= P.exposure; }
      if (stage_gas & use_prob) {
        const double prob = gas_conversion_prob(dm2_abs, gas, term1, L.sincos, cos_lead);
        w *= prob;
        till_m &= ballot64(prob != 0.0);
      }
      const uint64_t passed_m = geo.m_chip & ballot64(w != 0.0);
      if (lane == 0) {
        if (passed_m) __hip_atomic_fetch_add(&lds.cnt[k][0], (uint32_t)__popcll(passed_m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (till_m) __hip_atomic_fetch_add(&lds.cnt[k][1], (uint32_t)__popcll(till_m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      if (__builtin_amdgcn_inverse_ballot_w64(passed_m)) {
        // cell [k][0][lane % 32], [k][1][.] kScanLanes further on (the mass scan's layout)
        const uint32_t t = (uint32_t)k * (2u * kScanLanes) + ((uint32_t)lane & (kScanLanes - 1u));
        if constexpr (FIXED) {
          __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(cell(t)), (unsigned long long)to_fixed(w, E.fx_scale_w),
                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(cell(t + kScanLanes)), (unsigned long long)to_fixed(w * w, E.fx_scale_w2),
                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
          __hip_atomic_fetch_add(cell(t), w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          __hip_atomic_fetch_add(cell(t + kScanLanes), w * w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
    }
    __builtin_amdgcn_s_setprio(0);
  };

  uint32_t chunk = (uint32_t)wave_global;
  const uint32_t lane4 = 4u * (uint32_t)lane;
  uint32_t pass = 0;
  U4 stream = U4{0u, 0u, 0u, 0u};
  for (;;) {
    const bool have_new = chunk < n_chunks;   // wave-uniform
    if (have_new) {
      if (pass == 0u) stream = stream_block(((first_chunk + (uint64_t)chunk) << 6) + (uint64_t)lane, A.seed_lo, A.seed_hi);
      const uint32_t w = word_of(stream, pass);
      const uint32_t rel = ((chunk << 8) + pass) + lane4;
      run_phase_a(rel, (rel >= rel_begin) & (rel < rel_end), w);
      pass = (pass + 1u) & 3u;
      if (pass == 0u) chunk += (uint32_t)waves_total;
      ring_sync();
    }
    const uint32_t n1 = t1 - h1;
    if ((n1 >= 64u) | (!have_new & (n1 > 0u))) {
      run_phase_b(min(n1, 64u));
      ring_sync();
    }
    if (!have_new & (t1 == h1)) break;
  }

  // per-energy sums of this workgroup: a wave adds up the cells of an energy (lanes 0 .. 31: sum of w, 32 .. 63: sum of w^2; a fixed
  // order) -> plain stores, folded by fold_escan_kernel
  using Sum = std::conditional_t<FIXED, long long, double>;
  if (lane == 0) {
    if (n_reached) atomicAdd(&lds.shared_cnt[0], n_reached);
    if (n_shell) atomicAdd(&lds.shared_cnt[1], n_shell);
    if (n_nickel) atomicAdd(&lds.shared_cnt[2], n_nickel);
  }
  __syncthreads();
  for (int k = wave; k < ENarg.n_energies; k += BLOCK / 64) {
    Sum* const dst = reinterpret_cast<Sum*>(ENarg.partials) + ((size_t)blockIdx.x * kEScanMaxEnergies + (size_t)k) * kScanPartialSlots;
    const double c = *cell((uint32_t)k * 64u + (uint32_t)lane);
    Sum v;
    if constexpr (FIXED) v = __double_as_longlong(c); else v = c;
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);   // within each half of the wave
    if (lane == 0) { dst[0] = v; dst[2] = (Sum)lds.cnt[k][0]; dst[3] = (Sum)lds.cnt[k][1]; }
    if (lane == 32) dst[1] = v;
  }
  if (threadIdx.x < 4) {
    Sum* const r = reinterpret_cast<Sum*>(A.partials) + (size_t)blockIdx.x * 4;
    r[threadIdx.x] = (Sum)lds.shared_cnt[threadIdx.x];
  }
  (void)unused; (void)HBarg;
}

// ------------------------------------------------------------------------------------------------
// fused angular scan (include/sart.h: sart_trace_angular_scan; BASELINE configs[3])
// ------------------------------------------------------------------------------------------------
// performAngularScan (:2778-2802) re-runs the whole trace per telescope angle.  The angle enters a ray at the transformation
// into the telescope's frame (:1878-1899) and nowhere before it: sampling, the three sincos, the radius draw, bore, cold-bore
// exit and pipe cuts (phase_a_bore: ~215 of phase A's ~365 vector instructions in the rotated variant, and all of stage A0) do
// not depend on it.  This kernel therefore takes every ray through stage A0 and the first half of phase A ONCE and keeps the
// full wave of rays that come out of it in registers (the "stash": 11 values per lane - x1, y1, x3, y3, path, energy index: the
// energy draw (:444-471: radius index and u5 -> lowerBound in the CDF row) does not depend on the angle either, so its two
// table gathers with the worst locality - guide word, CDF candidates - are paid once per ray, not once per ray and angle);
// a wave-uniform walk over the launch's angles runs the second half of phase A (phase_a_telescope with that angle's rotation,
// read from the kernel arguments with scalar loads) on the stash, compacts the survivors into ring 1 with their angle index, and
// phase B runs on full waves of ring 1 as in the histogram kernel - a pass usually holds rays of two or three angles, so what
// phase B needs of the angle (the third column of the rotation, for z of pointExitCB) comes from a small LDS table per lane and
// the sums go to per-angle LDS cells (ds_add_f64 / ds_add_u64; ring 1's u5 column, free here) and counters (ds_add_u32).  No image,
// no position sums.
// One loop iteration runs at most one pass of each stage (one call site each: the instruction footprint of the histogram kernel):
//   no stash (ka == n_angles):  A0 pass -> ring 0;  ring 0 holds a full wave (or the input is exhausted) -> A1a -> stash, ka = 0
//   stash (ka < n_angles):      A1b for angle ka -> ring 1, ++ka
//   ring 1 holds a full wave (or everything before it has drained) -> B
// Same rays for every angle (common random numbers), the ray ids and uniforms of the histogram kernels: per angle the sums
// equal a sart_trace_histogram launch with that angle set on the same ray ids - bit for bit in SART_ACCUM_FIXED64.
// FAST / GAS as in trace_histogram_kernel (the telescope is always "rotated" here: angle 0 runs through the same arithmetic
// with cos = 1, sin = 0).
struct AScanKernArgs {
  HotA H;
  const DevBlob* blob;
  TraceArgs A;
  double* unused;      // (keeps the argument offsets of trace_histogram_kernel: the reload_* helpers are shared)
  HotB HB;
  AScanArgs AN;
};
static_assert(offsetof(AScanKernArgs, A) == offsetof(HistKernArgs, A) && offsetof(AScanKernArgs, HB) == offsetof(HistKernArgs, HB) &&
                  offsetof(AScanKernArgs, AN) == offsetof(HistKernArgs, SC) && sizeof(AScanAngle) % 8 == 0,
              "the angular-scan kernel re-reads its arguments at the offsets of the histogram kernel's");
constexpr int kAScanCells = kAScanMaxAngles * 2 * kScanLanes;          // [angle][sum w, sum w^2][kScanLanes]: ring 1's u5 column, 128 doubles per wave
constexpr int kAScanMTable = 0;                                        // [angle][mx, my, mz] in the cells behind the tables (the histogram kernels' tile_extra)
constexpr int kAScanCounters = 3 * kAScanMaxAngles;                    // behind it: (4 kAScanMaxAngles + 4) u32
static_assert(kAScanMTable + 3 * kAScanMaxAngles + (4 * kAScanMaxAngles + 4 + 1) / 2 <= kRingExtraCells, "rotation columns + counters live where the histogram kernels keep the image tile behind the tables");
static_assert(2 * kScanLanes == 64, "one cell per lane in the epilogue");
// ascan_images_kernel only, behind the counters in the same cells: [angle][SUM_X, SUM_Y, SUM_R][kAImgLanes] f64 / int64 (lanes l, l + 8,
// ... share a cell), [angle] SUM_WEIGHTS_OUTSIDE (FIXED), [angle] N_OUTSIDE_IMAGE (u32)
constexpr int kAImgLanes = 8;
constexpr int kAImgPos = kAScanCounters + (4 * kAScanMaxAngles + 4 + 1) / 2;
constexpr int kAImgOutside = kAImgPos + 3 * kAImgLanes * kAScanMaxAngles;
constexpr int kAImgNOutside = kAImgOutside + kAScanMaxAngles;
constexpr int kAImgCellsEnd = kAImgNOutside + kAScanMaxAngles / 2;
static_assert(kAImgCellsEnd <= kRingExtraCells && kAImgCellsEnd - kAImgPos <= 1024, "the image scan's sums fit the cells behind the tables");
static_assert(3 * kAImgLanes == 24, "one cell per lane of lanes 0 .. 23 in the epilogue");

// (The body is sart_angular_scan.inc: the image scan's kernel below shares the text, so that its rows are this kernel's bit for bit.)
template <int BLOCK, bool FAST, int GAS, bool FIXED>
__global__ __launch_bounds__(BLOCK) void trace_angular_scan_kernel(HotA H, const DevBlob* __restrict__ blob, TraceArgs A,
                                                                   double* __restrict__ img_partials, HotB HBarg, AScanArgs ANarg) {
  constexpr bool IMAGES = false;   // (img_partials: null, not read)
#include "sart_angular_scan.inc"
}

// Fused angular scan with per-angle images (include/sart.h: sart_trace_angular_scan_images_device): the scan above, and behind the
// weight of every passed (ray, angle) what trace_histogram_kernel accumulates for it - pixel, position sums, outside count and sum,
// spectra - into the angle's own accumulator block.  Same arguments at the same offsets (the reload_* helpers are shared); the
// fourth one receives the per-workgroup scalars [kAScanMaxAngles][n_blocks][SART_ACC_COUNT].
template <int BLOCK, bool FAST, int GAS, bool FIXED>
__global__ __launch_bounds__(BLOCK) void ascan_images_kernel(HotA H, const DevBlob* __restrict__ blob, TraceArgs A,
                                                             double* __restrict__ img_partials, HotB HBarg, AScanArgs ANarg) {
  constexpr bool IMAGES = true;
#include "sart_angular_scan.inc"
}

// What the finalize kernels report about a raw SART_ACCUM_FIXED64 accumulator (OR-ed into a word of the context that the next
// sart_synchronize reads): integers that no longer mean what they should.
constexpr uint32_t kFixedStatusWrapped = 1u;       // a slot is negative or >= 2^62: wrapped, or about to (weights and counts are >= 0)
constexpr uint32_t kFixedStatusUnresolved = 2u;    // the accumulated weights average below 2^12 quanta per passed ray
constexpr uint32_t kFixedStatusNotConserved = 4u;  // pixels (+ outside) / radial / energy weight bins do not add up to SUM_WEIGHTS: a slot wrapped

// ---- The limb arithmetic of every fold and finalize ("One fold tree, one limb arithmetic") ----
// A two-limb sum is value = hi * 2^40 + lo (include/sart.h), lo in the slot SART_*_SUM_*, hi in its *_HI slot.  FIXED = false is the
// f64 form of the same step: no limbs, hi stays 0.
constexpr long long kLimbMask = (1ll << kFixedLimbBits) - 1;
template <bool FIXED>
using FoldSum = std::conditional_t<FIXED, long long, double>;
// (lo, hi) += p, split before it is added: the workgroup partials are < 2^62 each, so nothing can wrap.  Arithmetic shift + mask:
// p = (p >> 40) * 2^40 + (p & mask) for negative p as well; an unsigned T (finalize_scan_bands_kernel) takes p modulo 2^64.
template <bool FIXED, class T>
__host__ __device__ __forceinline__ void limb_add(T& lo, T& hi, T p) {
  if constexpr (FIXED) { lo += p & (T)kLimbMask; hi += p >> kFixedLimbBits; } else lo += p;
}
// lo into [0, 2^40), the rest into hi
template <class T>
__host__ __device__ __forceinline__ void limbs_normalise(T& lo, T& hi) {
  const T l = lo;
  lo = 0;
  limb_add<true>(lo, hi, l);
}
template <class T>
__host__ __device__ __forceinline__ bool limbs_equal(T alo, T ahi, T blo, T bhi) {
  limbs_normalise(alo, ahi);
  limbs_normalise(blo, bhi);
  return alo == blo && ahi == bhi;
}
// hi * 2^40 and lo are exact doubles (below 2^53 each): one rounding in the sum
__device__ __forceinline__ double limbs_to_double(long long lo, long long hi) {
  const double two40 = (double)(1ll << kFixedLimbBits);
  return (double)hi * two40 + (double)lo;
}
// The two stores a fold ends with.  A plain counter:
template <bool FIXED, class Sum>
__device__ __forceinline__ void fold_add_counter(Sum* dst, Sum lo, Sum hi) {
  if constexpr (FIXED) *dst += (hi << kFixedLimbBits) + lo; else *dst += lo;
}
// ... and a two-limb sum, whose low limb is left in [0, 2^40) (lo + *lo_dst < 2^40 + 2^14 * 2^40)
template <bool FIXED, class Sum>
__device__ __forceinline__ void fold_add_pair(Sum* lo_dst, Sum* hi_dst, Sum lo, Sum hi) {
  if constexpr (FIXED) {
    hi += *hi_dst;
    lo += *lo_dst;
    limbs_normalise(lo, hi);
    *lo_dst = lo;
    *hi_dst = hi;
  } else {
    *lo_dst += lo;
  }
}
// slot s of `row`: a two-limb sum with its high limb in slot sh, or (sh < 0) a plain counter
template <bool FIXED, class Sum>
__device__ __forceinline__ void fold_store(Sum* row, int s, int sh, Sum lo, Sum hi) {
  if (sh >= 0) fold_add_pair<FIXED>(row + s, row + sh, lo, hi); else fold_add_counter<FIXED>(row + s, lo, hi);
}
// The resolution rules of the finalizes.  false: the squared weights average below 2^6 quanta per passed ray - the integers do not
// resolve them (their quantum 2^-39 of the squared weight bound is as fine as an int64 per workgroup allows); SUM_WEIGHTS_SQ - an error
// estimate, nothing else depends on it - then reads NaN in the f64 output instead of a number that looks like one.  The weights: below
// 2^12 quanta per passed ray.
// Both means are judged only once kFixedMinRaysForMeans rays have passed: the check is there to catch a weight BOUND that is off by
// orders of magnitude (an outlier in a table), and the average of a handful of rays says nothing about that - one faint ray alone
// in an accumulator (a launch of a single low-energy CAST ray, weight 1e-8 of the bound) is exact to half a quantum like every
// other and no reason to fail the call (found by the round-6 stream: ray 0 of seed 5 is such a ray).
constexpr double kFixedMinRaysForMeans = 256.0;
__device__ __forceinline__ bool squares_resolved(double n_passed, double sw2) {
  return !(n_passed >= kFixedMinRaysForMeans) || sw2 >= 64.0 * n_passed;
}
__device__ __forceinline__ bool weights_resolved(double n_passed, double sw) {
  return !(n_passed >= kFixedMinRaysForMeans) || sw >= 4096.0 * n_passed;
}
// Block-level sums of the finalizes.  Every thread of a wave calls these: *dst (LDS or global) += the wave's sum of v ...
__device__ __forceinline__ void wave_add_i64(long long v, long long* dst) {
  v = wave_sum_i64(v);
  if ((threadIdx.x & 63) == 0 && v != 0) atomicAdd(reinterpret_cast<unsigned long long*>(dst), (unsigned long long)v);
}
// ... and the limb pair (*lo_dst, *hi_dst) += the wave's sum of the pairs (lo, hi), normalised (a thread's few slots: no overflow)
__device__ __forceinline__ void wave_add_limbs(long long lo, long long hi, long long* lo_dst, long long* hi_dst) {
  lo = wave_sum_i64(lo);
  hi = wave_sum_i64(hi);
  if ((threadIdx.x & 63) != 0) return;
  limbs_normalise(lo, hi);
  if (lo != 0) atomicAdd(reinterpret_cast<unsigned long long*>(lo_dst), (unsigned long long)lo);
  if (hi != 0) atomicAdd(reinterpret_cast<unsigned long long*>(hi_dst), (unsigned long long)hi);
}

// ---- The fold tree ----
// A fold block is GROUPS x SLOTS threads; thread (g, slot) with `has` (its slot has partials) sums load(g), load(g + GROUPS), ... in
// that order, and the slot's first thread (g == 0) then adds the GROUPS group sums in order: the summation tree is fixed for a given
// grid.  Returns that total in (lo, hi) to the threads with g == 0 and `has`, zeros to the others.  EVERY thread of the block must
// call it (a barrier inside; the scan folds call it twice, pairs then counter rows, and so pass two).  `red`: the caller's LDS, one
// plane per limb.  FIXED says whether the partials are split at 2^40, not what Sum is: false is a plain sum - the f64 partials, and
// also the int64 counter rows of the scans in FIXED64, which need no limbs.
template <bool FIXED, int GROUPS, int SLOTS, class Sum, class Load>
__device__ __forceinline__ void fold_groups(Sum (&red)[FIXED ? 2 : 1][GROUPS][SLOTS], int g, int slot, int n_blocks, bool has, Load load,
                                            Sum& lo, Sum& hi) {
  lo = 0; hi = 0;
  if (has) {
    for (int b = g; b < n_blocks; b += GROUPS) limb_add<FIXED>(lo, hi, (Sum)load(b));
    red[0][g][slot] = lo;
    if constexpr (FIXED) red[1][g][slot] = hi;
  }
  __syncthreads();
  lo = 0; hi = 0;
  if (has && g == 0)
    for (int i = 0; i < GROUPS; ++i) {
      lo += red[0][i][slot];
      if constexpr (FIXED) hi += red[1][i][slot];
    }
}

// Fused angular scan: rows of the scan accumulator (include/sart.h: SART_ASCAN_*) += the per-workgroup sums of one launch.
// 1024 threads = 256 (angle, partial slot) pairs x 4 groups of workgroups (fold_groups).  `shared_row` (first group of angles of a
// scan only, else nullptr): the angle-independent counters.
template <bool FIXED>
__global__ __launch_bounds__(1024) void fold_ascan_kernel(double* __restrict__ rows_, double* __restrict__ shared_row_, const double* __restrict__ partials_,
                                                         int n_blocks, int n_angles, double n_rays) {
  using Sum = FoldSum<FIXED>;
  constexpr int kPairs = kAScanMaxAngles * kAScanPartialSlots, kGroups = 1024 / kPairs;
  static_assert(kPairs * kGroups == 1024 && kGroups >= 1, "one thread per (angle, partial slot, group of workgroups)");
  Sum* const rows = reinterpret_cast<Sum*>(rows_);
  Sum* const shared_row = reinterpret_cast<Sum*>(shared_row_);
  const Sum* const part = reinterpret_cast<const Sum*>(partials_);
  __shared__ Sum red[FIXED ? 2 : 1][kGroups][kPairs];
  const int pair = threadIdx.x % kPairs, g = threadIdx.x / kPairs;
  const int k = pair / kAScanPartialSlots, j = pair % kAScanPartialSlots;
  Sum lo, hi;
  fold_groups<FIXED, kGroups, kPairs>(red, g, pair, n_blocks, k < n_angles && j < 7,
                                      [&](int b) { return part[((size_t)b * kAScanMaxAngles + k) * kAScanPartialSlots + j]; }, lo, hi);
  if (g != 0) return;
  // partial slots 0 / 1 are the sums, 2 .. 5 the angle's counters, 6 (angle 0) the rays that reached the telescope
  if (k < n_angles && j < 6) {
    const int s = j == 0 ? SART_ASCAN_SUM_WEIGHTS : j == 1 ? SART_ASCAN_SUM_WEIGHTS_SQ : j == 2 ? SART_ASCAN_N_PASSED
                  : j == 3 ? SART_ASCAN_N_HIT_NICKEL : j == 4 ? SART_ASCAN_N_PASSED_TILL_WINDOW : SART_ASCAN_N_SHELL_SELECTED;
    fold_store<FIXED>(rows + (size_t)k * SART_ASCAN_ROW, s, j == 0 ? SART_ASCAN_SUM_WEIGHTS_HI : j == 1 ? SART_ASCAN_SUM_WEIGHTS_SQ_HI : -1, lo, hi);
  }
  if (shared_row && k == 0 && j == 6) fold_add_counter<FIXED>(&shared_row[SART_ASCAN_N_REACHED_TELESCOPE], lo, hi);
  if (shared_row && pair == 7) shared_row[SART_ASCAN_N_RAYS] += (Sum)n_rays;
}

// acc scalars += sum over workgroups of the partials; N_RAYS += n_rays.  256 threads: 8 groups x 32 quantity slots (24 used).  In
// SART_ACCUM_FIXED64 the five sums every passed ray of every launch adds to, and the weight outside the image, are two-limb sums: slot
// k's thread owns slot k and its *_HI slot; the threads of the *_HI slots (whose partials are zero) write nothing.
__device__ __forceinline__ int fixed_hi_slot(int k) {
  return k == SART_ACC_SUM_WEIGHTS ? SART_ACC_SUM_WEIGHTS_HI : k == SART_ACC_SUM_X ? SART_ACC_SUM_X_HI
         : k == SART_ACC_SUM_Y ? SART_ACC_SUM_Y_HI : k == SART_ACC_SUM_R ? SART_ACC_SUM_R_HI
         : k == SART_ACC_SUM_WEIGHTS_SQ ? SART_ACC_SUM_WEIGHTS_SQ_HI : k == SART_ACC_SUM_WEIGHTS_OUTSIDE ? SART_ACC_SUM_WEIGHTS_OUTSIDE_HI : -1;
}
__device__ __forceinline__ bool fixed_is_hi_slot(int k) {
  return (k >= SART_ACC_SUM_WEIGHTS_HI && k <= SART_ACC_SUM_R_HI) || k == SART_ACC_SUM_WEIGHTS_SQ_HI || k == SART_ACC_SUM_WEIGHTS_OUTSIDE_HI;
}
template <bool FIXED>
__device__ __forceinline__ void fold_scalars(FoldSum<FIXED>* __restrict__ scalars, const FoldSum<FIXED>* __restrict__ partials, int n_blocks,
                                             FoldSum<FIXED> n_rays) {
  using Sum = FoldSum<FIXED>;
  static_assert(SART_ACC_COUNT <= 32, "layout of the reduction below");
  __shared__ Sum red[FIXED ? 2 : 1][8][32];
  const int k = threadIdx.x & 31, g = threadIdx.x >> 5;
  Sum lo, hi;
  fold_groups<FIXED, 8, 32>(red, g, k, n_blocks, k < SART_ACC_COUNT, [&](int b) { return partials[(size_t)b * SART_ACC_COUNT + k]; }, lo, hi);
  if (g != 0 || k >= SART_ACC_COUNT || (FIXED && fixed_is_hi_slot(k))) return;
  if (k == SART_ACC_N_RAYS) lo += n_rays;   // (a plain counter, whose partials are zero: the fold adds the launch's rays)
  fold_store<FIXED>(scalars, k, fixed_hi_slot(k), lo, hi);
}
__global__ __launch_bounds__(256) void fold_scalars_kernel(double* __restrict__ scalars, const double* __restrict__ partials,
                                                           int n_blocks, double n_rays) {
  fold_scalars<false>(scalars, partials, n_blocks, n_rays);
}
__global__ __launch_bounds__(256) void fold_scalars_fixed_kernel(long long* __restrict__ scalars, const long long* __restrict__ partials,
                                                                 int n_blocks, long long n_rays) {
  fold_scalars<true>(scalars, partials, n_blocks, n_rays);
}

// acc[i] += sum over replicas; replicas are left zeroed for the next launch.  T = double, or long long (SART_ACCUM_FIXED64).
template <typename T>
__global__ __launch_bounds__(256) void fold_replicas_kernel(T* __restrict__ acc, T* __restrict__ replicas, int n_img,
                                                            int n_replicas, uint32_t stride) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_img) return;
  T s = 0;
  for (int r = 0; r < n_replicas; ++r) {
    s += replicas[(size_t)r * (size_t)stride + i];
    replicas[(size_t)r * (size_t)stride + i] = 0;
  }
  acc[i] += s;
}

// Fused mass scan: rows of the scan accumulator (include/sart.h: SART_SCAN_*) += the per-workgroup sums of one launch.
// 1024 threads = 128 (mass, quantity) pairs x 8 groups of workgroups (fold_groups).  Pair (k, 2) turns the counts into N_PASSED of
// mass k = rays with a non-zero mass-independent weight factor minus those whose conversion probability for this mass is exactly
// zero.  `shared_row` (first group of masses of a scan only, else nullptr): the mass-independent counters, plain sums of the
// workgroups' scalars through the same tree.
template <bool FIXED>
__global__ __launch_bounds__(1024) void fold_scan_kernel(double* __restrict__ rows_, double* __restrict__ shared_row_, const double* __restrict__ scal_partials_,
                                                        const double* __restrict__ scan_partials_, int n_blocks, int n_masses, double n_rays) {
  using Sum = FoldSum<FIXED>;
  constexpr int kPairs = kScanMaxMasses * kScanPartialSlots, kGroups = 8;
  static_assert(kPairs * kGroups == 1024, "one thread per (mass, partial slot, group of workgroups)");
  Sum* const rows = reinterpret_cast<Sum*>(rows_);
  Sum* const shared_row = reinterpret_cast<Sum*>(shared_row_);
  const Sum* const scal = reinterpret_cast<const Sum*>(scal_partials_);
  const Sum* const scan = reinterpret_cast<const Sum*>(scan_partials_);
  __shared__ Sum red[FIXED ? 2 : 1][kGroups][kPairs], red_cnt[1][kGroups][4];
  const int pair = threadIdx.x % kPairs, g = threadIdx.x / kPairs;
  const int k = pair >> 2, j = pair & 3;
  Sum lo, hi, cnt, none;
  fold_groups<FIXED, kGroups, kPairs>(red, g, pair, n_blocks, k < n_masses && j < 3, [&](int b) {
    const Sum p = scan[((size_t)b * kScanMaxMasses + k) * kScanPartialSlots + j];
    return j == 2 ? scal[(size_t)b * SART_ACC_COUNT + SART_ACC_N_PASSED] - p : p;
  }, lo, hi);
  // the four counters that come from the workgroup partials
  const int src = pair == 0 ? SART_ACC_N_REACHED_TELESCOPE : pair == 1 ? SART_ACC_N_SHELL_SELECTED : pair == 2 ? SART_ACC_N_HIT_NICKEL : SART_ACC_N_PASSED;
  fold_groups<false, kGroups, 4>(red_cnt, g, pair, n_blocks, shared_row && pair < 4, [&](int b) { return scal[(size_t)b * SART_ACC_COUNT + src]; }, cnt, none);
  if (g != 0) return;
  if (k < n_masses && j < 3)
    fold_store<FIXED>(rows + (size_t)k * SART_SCAN_ROW, j == 0 ? SART_SCAN_SUM_WEIGHTS : j == 1 ? SART_SCAN_SUM_WEIGHTS_SQ : SART_SCAN_N_PASSED,
                      j == 0 ? SART_SCAN_SUM_WEIGHTS_HI : j == 1 ? SART_SCAN_SUM_WEIGHTS_SQ_HI : -1, lo, hi);
  if (shared_row && pair < 4) {
    const int dst = pair == 0 ? SART_SCAN_N_REACHED_TELESCOPE : pair == 1 ? SART_SCAN_N_SHELL_SELECTED : pair == 2 ? SART_SCAN_N_HIT_NICKEL : SART_SCAN_N_ON_DETECTOR;
    shared_row[dst] += cnt;
    if (pair == 0) shared_row[SART_SCAN_N_RAYS] += (Sum)n_rays;
  }
}

// Banded mass scan: blocks of the spectra accumulator (include/sart.h: SART_MSPEC_*) += the per-workgroup band cells of one launch.
// One workgroup per mass of the group and, if `counts` (first group of masses of a scan only, else nullptr), one more for the
// per-band counts.  1024 threads = 64 cells (sum of w of band 0 .. 31, then sum of w^2) x 16 groups of workgroups (fold_groups).
// `block0`: the block of the group's first mass; n_cells = n_bands + 1 (cells behind them hold zeros and are not stored).
template <bool FIXED>
__global__ __launch_bounds__(1024) void fold_scan_bands_kernel(double* __restrict__ block0_, double* __restrict__ counts_, const double* __restrict__ band_partials_,
                                                              int n_blocks, int n_masses, int n_cells) {
  using Sum = FoldSum<FIXED>;
  constexpr int kCells = 2 * kScanLanes, kGroups = 16;
  static_assert(kCells * kGroups == 1024, "one thread per (cell, group of workgroups)");
  const Sum* const part = reinterpret_cast<const Sum*>(band_partials_);
  __shared__ Sum red[FIXED ? 2 : 1][kGroups][kCells];
  const int c = threadIdx.x % kCells, g = threadIdx.x / kCells;
  const int k = blockIdx.x;   // mass of the group, or n_masses: the counts
  const bool is_counts = k == n_masses;
  const int row = is_counts ? kScanMaxMasses : k;
  const int band = c & (kScanLanes - 1);
  const bool mine = band < n_cells && !(is_counts && c >= kScanLanes);
  Sum lo, hi;
  fold_groups<FIXED, kGroups, kCells>(red, g, c, n_blocks, mine,
                                      [&](int b) { return part[((size_t)b * (kScanMaxMasses + 1) + (size_t)row) * kCells + c]; }, lo, hi);
  if (g != 0 || !mine) return;
  if (is_counts) {
    fold_add_counter<FIXED>(reinterpret_cast<Sum*>(counts_) + (size_t)band * SART_MSPEC_CELL + SART_MSPEC_N_ON_DETECTOR, lo, hi);
    return;
  }
  Sum* const dst = reinterpret_cast<Sum*>(block0_) + ((size_t)k * (size_t)n_cells + (size_t)band) * SART_MSPEC_CELL;
  if (c < kScanLanes) fold_add_pair<FIXED>(dst + SART_MSPEC_SUM_WEIGHTS, dst + SART_MSPEC_SUM_WEIGHTS_HI, lo, hi);
  else fold_add_pair<FIXED>(dst + SART_MSPEC_SUM_WEIGHTS_SQ, dst + SART_MSPEC_SUM_WEIGHTS_SQ_HI, lo, hi);
}

// Fused energy scan: rows of the scan accumulator (include/sart.h: SART_ESCAN_*) += the per-workgroup sums of one launch.  1024
// threads = 128 (energy, quantity) pairs x 8 groups of workgroups (fold_groups).  `shared_row` (first group of energies of a scan
// only, else nullptr): the energy-independent counters from shared_partials[n_blocks][4].
template <bool FIXED>
__global__ __launch_bounds__(1024) void fold_escan_kernel(double* __restrict__ rows_, double* __restrict__ shared_row_,
                                                          const double* __restrict__ shared_partials_, const double* __restrict__ escan_partials_,
                                                          int n_blocks, int n_energies, double n_rays) {
  using Sum = FoldSum<FIXED>;
  constexpr int kPairs = kEScanMaxEnergies * kScanPartialSlots, kGroups = 8;
  static_assert(kPairs * kGroups == 1024, "one thread per (energy, partial slot, group of workgroups)");
  Sum* const rows = reinterpret_cast<Sum*>(rows_);
  Sum* const shared_row = reinterpret_cast<Sum*>(shared_row_);
  const Sum* const shp = reinterpret_cast<const Sum*>(shared_partials_);
  const Sum* const esp = reinterpret_cast<const Sum*>(escan_partials_);
  __shared__ Sum red[FIXED ? 2 : 1][kGroups][kPairs], red_cnt[1][kGroups][4];
  const int pair = threadIdx.x % kPairs, g = threadIdx.x / kPairs;
  const int k = pair >> 2, j = pair & 3;
  Sum lo, hi, cnt, none;
  fold_groups<FIXED, kGroups, kPairs>(red, g, pair, n_blocks, k < n_energies,
                                      [&](int b) { return esp[((size_t)b * kEScanMaxEnergies + k) * kScanPartialSlots + j]; }, lo, hi);
  fold_groups<false, kGroups, 4>(red_cnt, g, pair, n_blocks, shared_row && pair < 3, [&](int b) { return shp[(size_t)b * 4 + pair]; }, cnt, none);
  if (g != 0) return;
  if (k < n_energies) {
    const int s = j == 0 ? SART_ESCAN_SUM_WEIGHTS : j == 1 ? SART_ESCAN_SUM_WEIGHTS_SQ : j == 2 ? SART_ESCAN_N_PASSED : SART_ESCAN_N_PASSED_TILL_WINDOW;
    fold_store<FIXED>(rows + (size_t)k * SART_ESCAN_ROW, s, j == 0 ? SART_ESCAN_SUM_WEIGHTS_HI : j == 1 ? SART_ESCAN_SUM_WEIGHTS_SQ_HI : -1, lo, hi);
  }
  if (shared_row && pair < 3) {
    const int dst = pair == 0 ? SART_ESCAN_N_REACHED_TELESCOPE : pair == 1 ? SART_ESCAN_N_SHELL_SELECTED : SART_ESCAN_N_HIT_NICKEL;
    shared_row[dst] += cnt;
    if (pair == 0) shared_row[SART_ESCAN_N_RAYS] += (Sum)n_rays;
  }
}

// Scratch of one finalize (device memory of the context; word 0 = the status, kept; the rest zeroed before every finalize): exact
// two-limb sums of the raw slots that must add up to SUM_WEIGHTS.  Every passed ray adds the SAME integer to SUM_WEIGHTS and to one
// pixel (or to SUM_WEIGHTS_OUTSIDE), one radial bin and one energy bin, so the equalities hold exactly - unless a slot wrapped,
// however often: each wrap takes 2^64 out of its sum.
struct FixedCheck {
  uint32_t status, _pad;
  long long pix_lo, pix_hi, rad_lo, rad_hi, en_lo, en_hi;   // sums over the slots
  long long want_in_lo, want_in_hi;                         // SUM_WEIGHTS - SUM_WEIGHTS_OUTSIDE
  long long want_lo, want_hi;                               // SUM_WEIGHTS
  long long spectra;
  // (not zeroed per finalize) the sums of the FIRST finalize whose conservation check failed, for the error message: which sum is
  // off, in which direction and by how much says whether a slot wrapped (a multiple of 2^64 quanta) or an update went astray
  long long fail[10];                                       // pix, want_in, rad, en, want: (lo, hi) each
};
__device__ __forceinline__ void fixed_check_add(long long v, long long v_hi, bool mine, long long* lo_dst, long long* hi_dst) {
  if (!__builtin_amdgcn_ballot_w64(mine)) return;   // wave-uniform
  // (v_hi: the slot's limb in the roll-over array, in units of 2^40 - sart_rollover_accumulator_device; 0 without one)
  long long lo = 0, hi = 0;
  if (mine) { hi = v_hi; limb_add<true>(lo, hi, v); }
  wave_add_limbs(lo, hi, lo_dst, hi_dst);
}
__global__ void fixed_check_kernel(FixedCheck* C) {
  bool ok = limbs_equal(C->pix_lo, C->pix_hi, C->want_in_lo, C->want_in_hi);
  if (C->spectra) ok = ok && limbs_equal(C->rad_lo, C->rad_hi, C->want_lo, C->want_hi) && limbs_equal(C->en_lo, C->en_hi, C->want_lo, C->want_hi);
  if (!ok) {
    if (!(C->status & kFixedStatusNotConserved)) {
      const long long v[10] = {C->pix_lo, C->pix_hi, C->want_in_lo, C->want_in_hi, C->rad_lo, C->rad_hi, C->en_lo, C->en_hi, C->want_lo, C->want_hi};
      for (int i = 0; i < 10; ++i) C->fail[i] = v[i];
    }
    atomicOr(&C->status, kFixedStatusNotConserved);
  }
}
__device__ __forceinline__ void fixed_status_check_slot(long long v, uint32_t* status) {
  if (v < 0 || v >= (1ll << 62)) atomicOr(status, kFixedStatusWrapped);
}
// Sets the status where the weights are not resolved; returns whether the squared weights are (squares_resolved)
__device__ __forceinline__ bool fixed_status_check_means(double quanta_w, double quanta_w2, double n_passed, uint32_t* status) {
  if (!weights_resolved(n_passed, quanta_w)) atomicOr(status, kFixedStatusUnresolved);
  return squares_resolved(n_passed, quanta_w2);
}

// Raw SART_ACCUM_FIXED64 accumulator -> the f64 layout of include/sart.h (sart_finalize_accumulator_device).  Element-wise, so
// `out` may alias `in`; the scalars are converted by one thread, which reads all of them before it writes.
struct FinalizeArgs {
  long long n_img;
  int32_t spectra, n_radial_bins, n_energies1, _pad;
  double q_w, q_w2, q_pos, q_refl;
};
// `hi` (or nullptr): the roll-over limbs of sart_rollover_accumulator_device - slot i then stands for hi[i] 2^40 + in[i].
__global__ __launch_bounds__(256) void finalize_fixed_kernel(const long long* in, const long long* hi, double* out, FinalizeArgs F, FixedCheck* C) {
  uint32_t* const status = &C->status;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long n_scalar0 = F.n_img, n_spec0 = F.n_img + SART_ACC_COUNT;
  const long long total = n_spec0 + (F.spectra ? 2ll * F.n_radial_bins + 3ll * F.n_energies1 : 0ll);
  const double two40 = (double)(1ll << kFixedLimbBits);
  {
    // conservation sums (whole waves take part: the block size divides into waves, the last block is padded with idle threads)
    const long long v = i < total ? in[i] : 0ll;
    const long long h = (hi && i < total) ? hi[i] : 0ll;
    const long long j = i - n_spec0, nr = F.n_radial_bins, ne = F.n_energies1;
    fixed_check_add(v, h, i < n_scalar0, &C->pix_lo, &C->pix_hi);
    if (F.spectra) {
      fixed_check_add(v, h, j >= nr && j < 2 * nr, &C->rad_lo, &C->rad_hi);
      fixed_check_add(v, h, j >= 2 * nr + ne && j < 2 * nr + 2 * ne, &C->en_lo, &C->en_hi);
    }
  }
  if (i < n_scalar0) {
    const long long v = in[i];
    fixed_status_check_slot(v, status);
    // power-of-two quantum: the product is exact; with a roll-over limb the sum of the two exact doubles rounds once
    out[i] = (hi ? fma((double)hi[i], two40, (double)v) : (double)v) * F.q_w;
  } else if (i == n_scalar0) {
    long long v[SART_ACC_COUNT];
    double vd[SART_ACC_COUNT];     // the slot's value with its roll-over limb
    for (int k = 0; k < SART_ACC_COUNT; ++k) {
      v[k] = in[n_scalar0 + k];
      fixed_status_check_slot(v[k], status);
      const long long h = hi ? hi[n_scalar0 + k] : 0ll;
      if (h < 0) atomicOr(status, kFixedStatusWrapped);
      vd[k] = hi ? fma((double)h, two40, (double)v[k]) : (double)v[k];
    }
    auto limbs = [&](int k, int kh) {                      // hi * 2^40 and lo are exact doubles: one rounding in the sum
      return vd[kh] * two40 + vd[k];
    };
    const bool sq_ok = fixed_status_check_means(limbs(SART_ACC_SUM_WEIGHTS, SART_ACC_SUM_WEIGHTS_HI),
                                                limbs(SART_ACC_SUM_WEIGHTS_SQ, SART_ACC_SUM_WEIGHTS_SQ_HI), vd[SART_ACC_N_PASSED], status);
    // SUM_WEIGHTS in units of the quantum as (lo, hi 2^40): its two slots, each with its roll-over limb (the limb of the *_HI slot
    // counts 2^80 quanta: only a sum beyond 2^102 quanta would not fit the int64 below)
    auto hi_of = [&](int k, int kh) {
      return v[kh] + (hi ? hi[n_scalar0 + k] + (hi[n_scalar0 + kh] << kFixedLimbBits) : 0ll);
    };
    C->want_lo = v[SART_ACC_SUM_WEIGHTS];
    C->want_hi = hi_of(SART_ACC_SUM_WEIGHTS, SART_ACC_SUM_WEIGHTS_HI);
    C->want_in_lo = v[SART_ACC_SUM_WEIGHTS] - v[SART_ACC_SUM_WEIGHTS_OUTSIDE];
    C->want_in_hi = C->want_hi - hi_of(SART_ACC_SUM_WEIGHTS_OUTSIDE, SART_ACC_SUM_WEIGHTS_OUTSIDE_HI);
    C->spectra = F.spectra;
    for (int k = 0; k < SART_ACC_COUNT; ++k) {
      double r;
      switch (k) {
        case SART_ACC_SUM_WEIGHTS: r = limbs(k, SART_ACC_SUM_WEIGHTS_HI) * F.q_w; break;
        case SART_ACC_SUM_X: r = limbs(k, SART_ACC_SUM_X_HI) * F.q_pos; break;
        case SART_ACC_SUM_Y: r = limbs(k, SART_ACC_SUM_Y_HI) * F.q_pos; break;
        case SART_ACC_SUM_R: r = limbs(k, SART_ACC_SUM_R_HI) * F.q_pos; break;
        case SART_ACC_SUM_WEIGHTS_SQ: r = sq_ok ? limbs(k, SART_ACC_SUM_WEIGHTS_SQ_HI) * F.q_w2 : __builtin_nan(""); break;
        case SART_ACC_SUM_WEIGHTS_OUTSIDE: r = 0.0; break;   // (a raw-accumulator slot: the f64 layout has none)
        default: r = fixed_is_hi_slot(k) ? 0.0 : vd[k]; break;   // counters (the reserved slots hold 0)
      }
      out[n_scalar0 + k] = r;
    }
  } else if (F.spectra && i >= n_spec0) {
    // radial_counts | radial_weights | energy_counts | energy_weights | energy_reflect
    const long long j = i - n_spec0, nr = F.n_radial_bins, ne = F.n_energies1;
    if (j < 2 * nr + 3 * ne) {
      const double q = j < nr ? 1.0 : j < 2 * nr ? F.q_w : j < 2 * nr + ne ? 1.0 : j < 2 * nr + 2 * ne ? F.q_w : F.q_refl;
      const long long v = in[i];
      fixed_status_check_slot(v, status);
      out[i] = (hi ? fma((double)hi[i], two40, (double)v) : (double)v) * q;
    }
  }
}

// sart_rollover_accumulator_device: the bits of every slot above 2^40 move into the slot's limb in `hi` (units of 2^40); the slot
// keeps [0, 2^40).  A slot that is negative or >= 2^62 has wrapped (or is about to): reported like the finalize kernel does.
__global__ __launch_bounds__(256) void rollover_fixed_kernel(long long* acc, long long* hi, long long n, FixedCheck* C) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  long long v = acc[i], h = hi[i];
  fixed_status_check_slot(v, &C->status);
  limbs_normalise(v, h);
  if (h < 0) atomicOr(&C->status, kFixedStatusWrapped);
  hi[i] = h;
  acc[i] = v;
}

// Raw FIXED64 scan accumulator -> doubles: rows [0, n) of `in` / `out` (a group of up to kScanMaxMasses masses, whose quanta
// travel in the kernel arguments) and, if `shared_row`, the counter row behind the whole scan.  One thread per row.
struct FinalizeScanArgs {
  int32_t n_masses, shared_row;    // shared_row: row index of the counters relative to `in`, or -1
  uint32_t counter_slots, _pad;    // bit j < 8: slot j of a row is a plain counter (mass scan: N_PASSED; angular scan: its four counters)
                                   // bit 31 (kFinalizeScanRowsUnresolvedNaN): see finalize_scan_kernel
  double q_w[kScanMaxMasses], q_w2[kScanMaxMasses];
};
// Unresolved weights (the row's SUM_WEIGHTS averages below 2^12 quanta per passed ray).  The mass scan has a quantum per mass, derived
// from that mass's own weight bound: an unresolved row there means the bound is off, and the whole scan reports
// SART_ERR_ACCUMULATOR.  The angular scan has ONE quantum for all its angles, from the on-axis weight bound - an angle far off axis
// can pass a few rays of tiny R1 R2 that it does not resolve while every other row is fine: with bit 31 of counter_slots that row's
// SUM_WEIGHTS reads NaN (as an unresolved SUM_WEIGHTS_SQ does everywhere) and the status stays clean.
__global__ __launch_bounds__(64) void finalize_scan_kernel(const long long* in, double* out, FinalizeScanArgs F, FixedCheck* C) {
  uint32_t* const status = &C->status;
  const int k = threadIdx.x;
  long long v[SART_SCAN_ROW];
  if (k < F.n_masses) {
    for (int j = 0; j < SART_SCAN_ROW; ++j) { v[j] = in[(size_t)k * SART_SCAN_ROW + j]; fixed_status_check_slot(v[j], status); }
    const double sw = limbs_to_double(v[SART_SCAN_SUM_WEIGHTS], v[SART_SCAN_SUM_WEIGHTS_HI]);
    const double sw2 = limbs_to_double(v[SART_SCAN_SUM_WEIGHTS_SQ], v[SART_SCAN_SUM_WEIGHTS_SQ_HI]);
    const double n_passed = (double)v[SART_SCAN_N_PASSED];
    bool w_ok = true, sq_ok;
    if (F.counter_slots >> 31) {
      w_ok = weights_resolved(n_passed, sw);
      sq_ok = squares_resolved(n_passed, sw2);
    } else {
      sq_ok = fixed_status_check_means(sw, sw2, n_passed, status);
    }
    double* const o = out + (size_t)k * SART_SCAN_ROW;
    for (int j = 0; j < SART_SCAN_ROW; ++j) o[j] = 0.0;
    o[SART_SCAN_SUM_WEIGHTS] = w_ok ? sw * F.q_w[k] : __builtin_nan("");
    o[SART_SCAN_SUM_WEIGHTS_SQ] = sq_ok ? sw2 * F.q_w2[k] : __builtin_nan("");
    for (int j = 0; j < SART_SCAN_ROW; ++j)
      if ((F.counter_slots >> j) & 1u) o[j] = (double)v[j];   // (SART_SCAN_ROW = 8: bit 31 is not a slot)
  } else if (k == 63 && F.shared_row >= 0) {
    for (int j = 0; j < SART_SCAN_ROW; ++j) { v[j] = in[(size_t)F.shared_row * SART_SCAN_ROW + j]; fixed_status_check_slot(v[j], status); }
    for (int j = 0; j < SART_SCAN_ROW; ++j) out[(size_t)F.shared_row * SART_SCAN_ROW + j] = (double)v[j];
  }
}

// Raw FIXED64 spectra of a banded mass scan -> doubles (include/sart.h: sart_finalize_mass_scan_spectra_device), for a group of up
// to kScanMaxMasses masses whose quanta travel in the kernel arguments.  One wave per mass, lane c = cell c; if `counts_in`, one more
// wave for the per-band counts.  `rows`: the RAW scan rows of the group, `shared_row` the raw counter row (finalize_scan_kernel
// converts and judges those; this kernel only reads them).  Checks: every slot in [0, 2^62); the cells of a mass add up to its scan
// row, both sums and both limbs, and the band counts to N_ON_DETECTOR - as integers modulo 2^64, which a wrapped slot breaks; a mass
// whose squared weights the row does not resolve (squares_resolved) reads NaN in every cell's sum of w^2.
struct FinalizeBandsArgs {
  int32_t n_masses, n_cells;
  double q_w[kScanMaxMasses], q_w2[kScanMaxMasses];
};
__global__ __launch_bounds__(64) void finalize_scan_bands_kernel(const long long* __restrict__ rows, const long long* __restrict__ shared_row,
                                                                 const long long* in, double* out, const long long* counts_in, double* counts_out,
                                                                 FinalizeBandsArgs F, FixedCheck* C) {
  using U = unsigned long long;
  uint32_t* const status = &C->status;
  const int k = blockIdx.x, c = threadIdx.x;
  const bool mine = c < F.n_cells;
  if (k == F.n_masses) {   // the counts
    long long v[SART_MSPEC_CELL] = {0, 0, 0, 0};
    if (mine) {
      for (int j = 0; j < SART_MSPEC_CELL; ++j) { v[j] = counts_in[(size_t)c * SART_MSPEC_CELL + j]; fixed_status_check_slot(v[j], status); }
    }
    const U total = wave_sum((U)v[SART_MSPEC_N_ON_DETECTOR]);
    if (c == 0 && total != (U)shared_row[SART_SCAN_N_ON_DETECTOR]) atomicOr(status, kFixedStatusNotConserved);
    if (mine)
      for (int j = 0; j < SART_MSPEC_CELL; ++j) counts_out[(size_t)c * SART_MSPEC_CELL + j] = j == SART_MSPEC_N_ON_DETECTOR ? (double)v[j] : 0.0;
    return;
  }
  const long long* const row = rows + (size_t)k * SART_SCAN_ROW;
  const bool sq_ok = squares_resolved((double)row[SART_SCAN_N_PASSED], limbs_to_double(row[SART_SCAN_SUM_WEIGHTS_SQ], row[SART_SCAN_SUM_WEIGHTS_SQ_HI]));
  long long v[SART_MSPEC_CELL] = {0, 0, 0, 0};
  const size_t at = ((size_t)k * (size_t)F.n_cells + (size_t)c) * SART_MSPEC_CELL;
  if (mine)
    for (int j = 0; j < SART_MSPEC_CELL; ++j) { v[j] = in[at + j]; fixed_status_check_slot(v[j], status); }
  // normalised limbs, summed over the cells
  U w_lo = 0, w_hi = (U)v[SART_MSPEC_SUM_WEIGHTS_HI], q_lo = 0, q_hi = (U)v[SART_MSPEC_SUM_WEIGHTS_SQ_HI];
  limb_add<true>(w_lo, w_hi, (U)v[SART_MSPEC_SUM_WEIGHTS]);
  limb_add<true>(q_lo, q_hi, (U)v[SART_MSPEC_SUM_WEIGHTS_SQ]);
  w_lo = wave_sum(w_lo); w_hi = wave_sum(w_hi);
  q_lo = wave_sum(q_lo); q_hi = wave_sum(q_hi);
  if (c == 0 && (!limbs_equal(w_lo, w_hi, (U)row[SART_SCAN_SUM_WEIGHTS], (U)row[SART_SCAN_SUM_WEIGHTS_HI]) ||
                 !limbs_equal(q_lo, q_hi, (U)row[SART_SCAN_SUM_WEIGHTS_SQ], (U)row[SART_SCAN_SUM_WEIGHTS_SQ_HI])))
    atomicOr(status, kFixedStatusNotConserved);
  if (mine) {
    out[at + SART_MSPEC_SUM_WEIGHTS] = limbs_to_double(v[SART_MSPEC_SUM_WEIGHTS], v[SART_MSPEC_SUM_WEIGHTS_HI]) * F.q_w[k];
    out[at + SART_MSPEC_SUM_WEIGHTS_SQ] =
        sq_ok ? limbs_to_double(v[SART_MSPEC_SUM_WEIGHTS_SQ], v[SART_MSPEC_SUM_WEIGHTS_SQ_HI]) * F.q_w2[k] : __builtin_nan("");
    out[at + SART_MSPEC_SUM_WEIGHTS_HI] = 0.0;
    out[at + SART_MSPEC_SUM_WEIGHTS_SQ_HI] = 0.0;
  }
}

// The folds of the breakdowns: block row blockIdx.x (include/sart.h: SART_SHELL_*, SART_CHAN_*, the head SART_ORIGIN_*) += the
// per-workgroup tables of one launch.  One workgroup per row, 64 threads = kSlots partial slots (the first kUsed of them used) x
// 64 / kSlots groups of workgroups (fold_groups); partial (b, row, j) sits at (b kMaxRows + row) kPartialSlots + j and goes to slot
// dst(j) of the row, a two-limb sum where hi(j) >= 0.
struct ShellFold {     // partial slots 0 .. 3 are the counters SART_SHELL_N_*, 4 / 5 the sums
  static constexpr int kSlots = 8, kUsed = kShellPartialSlots, kPartialSlots = kShellPartialSlots, kMaxRows = kMaxShells, kRow = SART_SHELL_ROW;
  static __device__ int dst(int j) { return j < 4 ? j : j == 4 ? SART_SHELL_SUM_WEIGHTS : SART_SHELL_SUM_WEIGHTS_SQ; }
  static __device__ int hi(int j) { return j == 4 ? SART_SHELL_SUM_WEIGHTS_HI : j == 5 ? SART_SHELL_SUM_WEIGHTS_SQ_HI : -1; }
};
struct ChannelFold {   // partial slots 0 .. 2 are the sums SUM_WEIGHTS, SUM_WEIGHTS_SQ, SUM_WEIGHTS_OUTSIDE, 3 the counter N_CONTRIBUTING
  static constexpr int kSlots = kChanPartialSlots, kUsed = 4, kPartialSlots = kChanPartialSlots, kMaxRows = kMaxChannels, kRow = SART_CHAN_ROW;
  static __device__ int dst(int j) {
    return j == 0 ? SART_CHAN_SUM_WEIGHTS : j == 1 ? SART_CHAN_SUM_WEIGHTS_SQ : j == 2 ? SART_CHAN_SUM_WEIGHTS_OUTSIDE : SART_CHAN_N_CONTRIBUTING;
  }
  static __device__ int hi(int j) {
    return j == 0 ? SART_CHAN_SUM_WEIGHTS_HI : j == 1 ? SART_CHAN_SUM_WEIGHTS_SQ_HI : j == 2 ? SART_CHAN_SUM_WEIGHTS_OUTSIDE_HI : -1;
  }
};
struct OriginFold {    // one row, the head (the aperture block's too): partial slot 0 is the counter N_PASSED, 1 / 2 the sums
  static constexpr int kSlots = kOriginPartialSlots, kUsed = 3, kPartialSlots = kOriginPartialSlots, kMaxRows = 1, kRow = SART_ORIGIN_HEAD;
  static __device__ int dst(int j) { return j == 0 ? SART_ORIGIN_N_PASSED : j == 1 ? SART_ORIGIN_SUM_WEIGHTS : SART_ORIGIN_SUM_WEIGHTS_SQ; }
  static __device__ int hi(int j) { return j == 1 ? SART_ORIGIN_SUM_WEIGHTS_HI : j == 2 ? SART_ORIGIN_SUM_WEIGHTS_SQ_HI : -1; }
};
template <bool FIXED, class B>
__device__ __forceinline__ void fold_breakdown(double* __restrict__ block_, const double* __restrict__ partials_, int n_blocks) {
  using Sum = FoldSum<FIXED>;
  constexpr int kGroups = 64 / B::kSlots;
  static_assert(B::kSlots * kGroups == 64 && B::kUsed <= B::kSlots && B::kUsed <= B::kPartialSlots, "one thread per (partial slot, group of workgroups)");
  const Sum* const part = reinterpret_cast<const Sum*>(partials_);
  __shared__ Sum red[FIXED ? 2 : 1][kGroups][B::kSlots];
  const int j = threadIdx.x % B::kSlots, g = threadIdx.x / B::kSlots;
  Sum lo, hi;
  fold_groups<FIXED, kGroups, B::kSlots>(red, g, j, n_blocks, j < B::kUsed,
                                         [&](int b) { return part[((size_t)b * B::kMaxRows + blockIdx.x) * B::kPartialSlots + j]; }, lo, hi);
  if (g == 0 && j < B::kUsed) fold_store<FIXED>(reinterpret_cast<Sum*>(block_) + (size_t)blockIdx.x * B::kRow, B::dst(j), B::hi(j), lo, hi);
}
template <bool FIXED>
__global__ __launch_bounds__(64) void fold_shells_kernel(double* __restrict__ block, const double* __restrict__ partials, int n_blocks) {
  fold_breakdown<FIXED, ShellFold>(block, partials, n_blocks);     // 8 groups
}
template <bool FIXED>
__global__ __launch_bounds__(64) void fold_channels_kernel(double* __restrict__ block, const double* __restrict__ partials, int n_blocks) {
  fold_breakdown<FIXED, ChannelFold>(block, partials, n_blocks);   // 16 groups
}
template <bool FIXED>
__global__ __launch_bounds__(64) void fold_origin_kernel(double* __restrict__ block, const double* __restrict__ partials, int n_blocks) {
  fold_breakdown<FIXED, OriginFold>(block, partials, n_blocks);    // 16 groups
}

// Raw FIXED64 shell block -> doubles (sart_finalize_shells_device).  One workgroup per shell: its row and, with spectra, its two
// energy arrays.  Each slot is read and written by the same thread (in place allowed).  Checks, as finalize_fixed_kernel and
// finalize_scan_kernel do them: every slot in [0, 2^62); the shell's weights resolved (its SUM_WEIGHTS_SQ reads NaN where the squared
// weights are not); and, with spectra, the exact conservation laws of the block itself - every passed ray of the shell adds the same
// integer to SUM_WEIGHTS and to one energy-weight bin, and 1 to N_PASSED and to one energy-count bin.
struct FinalizeShellsArgs {
  int32_t n_shells, n_energies1, spectra, _pad;
  double q_w, q_w2;
};
__global__ __launch_bounds__(256) void finalize_shells_kernel(const long long* in, double* out, FinalizeShellsArgs F, FixedCheck* C) {
  uint32_t* const status = &C->status;
  const int s = blockIdx.x;
  const long long* const row = in + (size_t)s * SART_SHELL_ROW;
  long long v[SART_SHELL_ROW];
  for (int j = 0; j < SART_SHELL_ROW; ++j) v[j] = row[j];   // (every thread: read before the block's first write)
  __shared__ long long cnt_sum, w_lo, w_hi;
  if (threadIdx.x == 0) { cnt_sum = 0; w_lo = 0; w_hi = 0; }
  __syncthreads();
  if (F.spectra) {
    const size_t ne = (size_t)F.n_energies1;
    const size_t c0 = (size_t)F.n_shells * SART_SHELL_ROW + (size_t)s * ne, w0 = c0 + (size_t)F.n_shells * ne;
    long long c = 0, lo = 0, hi = 0;
    for (size_t e = threadIdx.x; e < ne; e += 256) {
      const long long n = in[c0 + e], w = in[w0 + e];
      fixed_status_check_slot(n, status);
      fixed_status_check_slot(w, status);
      c += n;
      limb_add<true>(lo, hi, w);
      out[c0 + e] = (double)n;
      out[w0 + e] = (double)w * F.q_w;
    }
    wave_add_i64(c, &cnt_sum);
    wave_add_limbs(lo, hi, &w_lo, &w_hi);
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int j = 0; j < SART_SHELL_ROW; ++j) fixed_status_check_slot(v[j], status);
  const double sw = limbs_to_double(v[SART_SHELL_SUM_WEIGHTS], v[SART_SHELL_SUM_WEIGHTS_HI]);
  const double sw2 = limbs_to_double(v[SART_SHELL_SUM_WEIGHTS_SQ], v[SART_SHELL_SUM_WEIGHTS_SQ_HI]);
  const bool sq_ok = fixed_status_check_means(sw, sw2, (double)v[SART_SHELL_N_PASSED], status);
  if (F.spectra && (cnt_sum != v[SART_SHELL_N_PASSED] || !limbs_equal(w_lo, w_hi, v[SART_SHELL_SUM_WEIGHTS], v[SART_SHELL_SUM_WEIGHTS_HI])))
    atomicOr(status, kFixedStatusNotConserved);
  double* const o = out + (size_t)s * SART_SHELL_ROW;
  for (int j = 0; j < SART_SHELL_ROW; ++j) o[j] = 0.0;
  o[SART_SHELL_N_SELECTED] = (double)v[SART_SHELL_N_SELECTED];
  o[SART_SHELL_N_HIT_NICKEL] = (double)v[SART_SHELL_N_HIT_NICKEL];
  o[SART_SHELL_N_PASSED_TILL_WINDOW] = (double)v[SART_SHELL_N_PASSED_TILL_WINDOW];
  o[SART_SHELL_N_PASSED] = (double)v[SART_SHELL_N_PASSED];
  o[SART_SHELL_SUM_WEIGHTS] = sw * F.q_w;
  o[SART_SHELL_SUM_WEIGHTS_SQ] = sq_ok ? sw2 * F.q_w2 : __builtin_nan("");
}

// Raw FIXED64 channel block -> doubles (sart_finalize_channels_device).  One workgroup per channel: its row, with spectra its energy
// bins, with an image its pixels.  Each slot is read and written by the same thread (in place allowed).  Checks: every slot in
// [0, 2^62); the exact conservation laws of the block itself - every contributing ray adds the same integer to SUM_WEIGHTS, to one
// energy bin and to one pixel or SUM_WEIGHTS_OUTSIDE.  No resolution check: a faint channel's c_t are exact to half a quantum of the
// total weight like every other, and its SUM_WEIGHTS_SQ is exact to N_CONTRIBUTING / 2 quanta of the squared weights.
struct FinalizeChannelsArgs {
  int32_t n_channels, n_energies1, spectra, _pad;
  long long n_img;
  double q_w, q_w2;
};
__global__ __launch_bounds__(256) void finalize_channels_kernel(const long long* in, double* out, FinalizeChannelsArgs F, FixedCheck* C) {
  uint32_t* const status = &C->status;
  const int t = blockIdx.x;
  const long long* const row = in + (size_t)t * SART_CHAN_ROW;
  long long v[SART_CHAN_ROW];
  for (int j = 0; j < SART_CHAN_ROW; ++j) v[j] = row[j];   // (every thread: read before the block's first write)
  __shared__ long long sums[4];   // energy bins lo, hi; pixels lo, hi
  if (threadIdx.x < 4) sums[threadIdx.x] = 0;
  __syncthreads();
  const size_t ne = (size_t)F.n_energies1, T = (size_t)F.n_channels;
  const size_t e0 = T * SART_CHAN_ROW + (size_t)t * ne;
  const size_t p0 = T * SART_CHAN_ROW + (F.spectra ? T * ne : (size_t)0) + (size_t)t * (size_t)F.n_img;
  long long acc4[4] = {0, 0, 0, 0};
  if (F.spectra)
    for (size_t e = threadIdx.x; e < ne; e += 256) {
      const long long w = in[e0 + e];
      fixed_status_check_slot(w, status);
      limb_add<true>(acc4[0], acc4[1], w);
      out[e0 + e] = (double)w * F.q_w;
    }
  for (size_t p = threadIdx.x; p < (size_t)F.n_img; p += 256) {
    const long long w = in[p0 + p];
    fixed_status_check_slot(w, status);
    limb_add<true>(acc4[2], acc4[3], w);
    out[p0 + p] = (double)w * F.q_w;
  }
  wave_add_limbs(acc4[0], acc4[1], &sums[0], &sums[1]);
  wave_add_limbs(acc4[2], acc4[3], &sums[2], &sums[3]);
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int j = 0; j < SART_CHAN_ROW; ++j) fixed_status_check_slot(v[j], status);
  const long long want_lo = v[SART_CHAN_SUM_WEIGHTS], want_hi = v[SART_CHAN_SUM_WEIGHTS_HI];
  if (F.spectra && !limbs_equal(sums[0], sums[1], want_lo, want_hi)) atomicOr(status, kFixedStatusNotConserved);
  if (!limbs_equal(sums[2] + v[SART_CHAN_SUM_WEIGHTS_OUTSIDE], sums[3] + v[SART_CHAN_SUM_WEIGHTS_OUTSIDE_HI], want_lo, want_hi))
    atomicOr(status, kFixedStatusNotConserved);
  double* const o = out + (size_t)t * SART_CHAN_ROW;
  for (int j = 0; j < SART_CHAN_ROW; ++j) o[j] = 0.0;
  o[SART_CHAN_SUM_WEIGHTS] = limbs_to_double(v[SART_CHAN_SUM_WEIGHTS], v[SART_CHAN_SUM_WEIGHTS_HI]) * F.q_w;
  o[SART_CHAN_SUM_WEIGHTS_SQ] = limbs_to_double(v[SART_CHAN_SUM_WEIGHTS_SQ], v[SART_CHAN_SUM_WEIGHTS_SQ_HI]) * F.q_w2;
  o[SART_CHAN_N_CONTRIBUTING] = (double)v[SART_CHAN_N_CONTRIBUTING];
  o[SART_CHAN_SUM_WEIGHTS_OUTSIDE] = limbs_to_double(v[SART_CHAN_SUM_WEIGHTS_OUTSIDE], v[SART_CHAN_SUM_WEIGHTS_OUTSIDE_HI]) * F.q_w;
}

// Raw FIXED64 origin block -> doubles (sart_finalize_origin_device), in two steps.  finalize_origin_kernel: the cells, one thread
// per cell in a grid-wide loop; each slot is read and written by the same thread (in place allowed), the head is only read (whether
// the squared weights are resolved: every SUM_WEIGHTS_SQ slot reads NaN where they are not).  Every slot must be in [0, 2^62), and the
// column sums of the cells - N, and the two sums in two limbs - go through a wave reduction to the context's FixedCheck scratch
// (pix: weights, rad: squared weights, en_lo: counts; zeroed by the host).  finalize_origin_head_kernel, behind it: the exact
// conservation laws of the block - every passed ray adds 1 to N_PASSED and to its cell's N, and the same two integers to the head's
// sums and to its cell's - and the head itself.
struct FinalizeOriginArgs {
  long long n_cells;
  double q_w, q_w2;
};
__global__ __launch_bounds__(256) void finalize_origin_kernel(const long long* in, double* out, FinalizeOriginArgs F, FixedCheck* C) {
  uint32_t* const status = &C->status;
  const bool sq_ok = squares_resolved((double)in[SART_ORIGIN_N_PASSED], limbs_to_double(in[SART_ORIGIN_SUM_WEIGHTS_SQ], in[SART_ORIGIN_SUM_WEIGHTS_SQ_HI]));
  long long cnt = 0, w_lo = 0, w_hi = 0, w2_lo = 0, w2_hi = 0;   // this thread's cells (a few: the limbs cannot overflow)
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < F.n_cells; i += stride) {
    const size_t o = (size_t)SART_ORIGIN_HEAD + (size_t)i * SART_ORIGIN_CELL;
    const long long n = in[o + SART_ORIGIN_N], w = in[o + SART_ORIGIN_SUM_WEIGHTS], w2 = in[o + SART_ORIGIN_SUM_WEIGHTS_SQ], r = in[o + 3];
    fixed_status_check_slot(n, status);
    fixed_status_check_slot(w, status);
    fixed_status_check_slot(w2, status);
    fixed_status_check_slot(r, status);
    cnt += n;
    limb_add<true>(w_lo, w_hi, w);
    limb_add<true>(w2_lo, w2_hi, w2);
    out[o + SART_ORIGIN_N] = (double)n;
    out[o + SART_ORIGIN_SUM_WEIGHTS] = (double)w * F.q_w;
    out[o + SART_ORIGIN_SUM_WEIGHTS_SQ] = sq_ok ? (double)w2 * F.q_w2 : __builtin_nan("");
    out[o + 3] = 0.0;
  }
  // (every thread is back here: whole waves reduce)
  wave_add_i64(cnt, &C->en_lo);
  wave_add_limbs(w_lo, w_hi, &C->pix_lo, &C->pix_hi);
  wave_add_limbs(w2_lo, w2_hi, &C->rad_lo, &C->rad_hi);
}
__global__ __launch_bounds__(64) void finalize_origin_head_kernel(const long long* in, double* out, FinalizeOriginArgs F, FixedCheck* C) {
  if (threadIdx.x != 0) return;
  uint32_t* const status = &C->status;
  long long v[SART_ORIGIN_HEAD];
  for (int j = 0; j < SART_ORIGIN_HEAD; ++j) { v[j] = in[j]; fixed_status_check_slot(v[j], status); }
  if (C->en_lo != v[SART_ORIGIN_N_PASSED] || !limbs_equal(C->pix_lo, C->pix_hi, v[SART_ORIGIN_SUM_WEIGHTS], v[SART_ORIGIN_SUM_WEIGHTS_HI]) ||
      !limbs_equal(C->rad_lo, C->rad_hi, v[SART_ORIGIN_SUM_WEIGHTS_SQ], v[SART_ORIGIN_SUM_WEIGHTS_SQ_HI]))
    atomicOr(status, kFixedStatusNotConserved);
  const double sw = limbs_to_double(v[SART_ORIGIN_SUM_WEIGHTS], v[SART_ORIGIN_SUM_WEIGHTS_HI]);
  const double sw2 = limbs_to_double(v[SART_ORIGIN_SUM_WEIGHTS_SQ], v[SART_ORIGIN_SUM_WEIGHTS_SQ_HI]);
  const bool sq_ok = squares_resolved((double)v[SART_ORIGIN_N_PASSED], sw2);
  for (int j = 0; j < SART_ORIGIN_HEAD; ++j) out[j] = 0.0;
  out[SART_ORIGIN_N_PASSED] = (double)v[SART_ORIGIN_N_PASSED];
  out[SART_ORIGIN_SUM_WEIGHTS] = sw * F.q_w;
  out[SART_ORIGIN_SUM_WEIGHTS_SQ] = sq_ok ? sw2 * F.q_w2 : __builtin_nan("");
}

// The fraction table of sart_set_source_channels[_device]: frac[cell stride + t] = rates[t][cell] / total[cell] (IEEE division; 0
// where total == 0), t >= T padded with 0, a fraction in (1, 1 + 2^-49] stored as 1.  One thread per cell (r, e).  *first_bad (set to
// ~0 by the host) = min over the offending entries of (cell 8 + t) 4 + code: 1 a negative or non-finite rate, 2 a fraction above
// 1 + 2^-49, 3 a negative or non-finite total (t = 0).
__global__ __launch_bounds__(256) void channel_fractions_kernel(const double* __restrict__ rates, const double* __restrict__ total,
                                                               double* __restrict__ frac, int n_channels, int stride, long long n_cells,
                                                               unsigned long long* first_bad) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_cells) return;
  const double tot = total[i];
  unsigned long long bad = ~0ull;
  if (!(tot >= 0.0) || !(tot <= 1.7976931348623157e308)) bad = ((unsigned long long)i * 8ull) * 4ull + 3ull;
  constexpr double kOneUp = 1.0 + 0x1p-49;
  for (int t = 0; t < stride; ++t) {
    double f = 0.0;
    if (t < n_channels) {
      const double r = rates[(size_t)t * (size_t)n_cells + (size_t)i];
      const unsigned long long key = ((unsigned long long)i * 8ull + (unsigned long long)t) * 4ull;
      if (!(r >= 0.0) || !(r <= 1.7976931348623157e308)) {
        bad = min(bad, key + 1ull);
      } else if (tot > 0.0) {
        f = r / tot;
        if (f > kOneUp) bad = min(bad, key + 2ull);
        f = fmin(f, 1.0);
      }
    }
    frac[(size_t)i * (size_t)stride + (size_t)t] = f;
  }
  if (bad != ~0ull) atomicMin(first_bad, bad);
}

// Literal drop-in for traceAxionWrapper: one Axion record per ray, in ray order (no compaction).
constexpr int kRecBlock = 256;
// `uniforms` != nullptr (sart_internal_trace_records_uniforms, a test entry): ray i takes its six uniforms from
// uniforms[6 i .. 6 i + 5] (draw order of SURVEY App. B) instead of from its Philox blocks - physics fixtures keyed by
// explicit uniforms survive a re-mapping of the random stream.
// The 26 eight-byte words of a record, in memory order: f(w, value), w a literal in every call.  The only list of them: what
// store_record writes and what the columns hold both come from here.  The two groups of byte-sized fields are packed by hand: a
// plain struct copy moves their padding arrays, too, and the compiler then keeps those bytes of the local record in scratch memory.
template <class F>
__device__ __forceinline__ void for_each_record_word(const sart_axion_t& r, F&& f) {
  static_assert(sizeof(sart_axion_t) == 208 && offsetof(sart_axion_t, pointdataX) == 8 && offsetof(sart_axion_t, kinds) == 128 &&
                    offsetof(sart_axion_t, transProbWindow) == 136 && offsetof(sart_axion_t, shellNumber) == 176,
                "layout of include/sart.h");
  auto bits = [](double v) { return (uint64_t)__double_as_longlong(v); };
  f(0u, (uint64_t)r.passed | ((uint64_t)r.passedTillWindow << 8) | ((uint64_t)r.hitNickel << 16));
  f(1u, bits(r.pointdataX)); f(2u, bits(r.pointdataY)); f(3u, bits(r.pointdataXBefore)); f(4u, bits(r.pointdataYBefore));
  f(5u, bits(r.pointdataR)); f(6u, bits(r.weights)); f(7u, bits(r.weightsAll)); f(8u, bits(r.transmissionMagnet));
  f(9u, bits(r.yawAngles)); f(10u, bits(r.pixvalsX)); f(11u, bits(r.pixvalsY)); f(12u, bits(r.radii));
  f(13u, bits(r.energiesAx)); f(14u, bits(r.energiesAxAll)); f(15u, bits(r.energiesAxWindow));
  f(16u, (uint64_t)r.kinds | ((uint64_t)r.kindsWindow << 8));
  f(17u, bits(r.transProbWindow)); f(18u, bits(r.transProbArgon)); f(19u, bits(r.transProbDetector)); f(20u, bits(r.transProbMagnet));
  f(21u, bits(r.deviationDet)); f(22u, (uint64_t)r.shellNumber); f(23u, bits(r.energiesPre)); f(24u, bits(r.emratesPre));
  f(25u, bits(r.reflect));
}
// One record to memory
__device__ __forceinline__ void store_record(sart_axion_t* dst, const sart_axion_t& r) {
  uint64_t* o = reinterpret_cast<uint64_t*>(dst);
  for_each_record_word(r, [&](uint32_t w, uint64_t v) { o[w] = v; });
}

// The record of ray i of the launch into rec, which the caller has zeroed: newSeq[Axion] zero-initialises (:2760)
__device__ __forceinline__ void record_of_ray(const HotA& H, const DevParams& P, const LdsTables& L, const HotB& HB, const TraceArgs& A,
                                              uint64_t i, const double* __restrict__ uniforms, sart_axion_t& rec) {
  RayState st;
  bool sampled, reached;
  double radial;    // not used here: the record path lets phase B find every miss itself (and so checks the shortcut of the histogram path)
  LaneMasks masks;  // not used here either: this body branches per lane on the bools
  const uint64_t ray_id = A.ray_id_offset + i;
  bool alive;
  if (uniforms) {   // wave-uniform
    const double* u = uniforms + 6 * i;
    const Uniforms U{u[0], u[1], u[2], u[3], u[4], u[5], upper32_of_uniform(u[2])};
    alive = phase_a_core<false, -1, false>(H, P, L, U, st, sampled, reached, radial, masks);
  } else {
    const uint32_t u3_hi = word_of(stream_block(ray_id >> 2, A.seed_lo, A.seed_hi), (uint32_t)ray_id & 3u);
    alive = phase_a<false, -1, false, false, false>(H, P, L, A.seed_lo, A.seed_hi, ray_id, u3_hi, st, sampled, reached, radial, masks);
  }
  int e_idx = -1;
  if (sampled) {
    e_idx = H.test_active ? P.n_energies : sample_energy_index(HB, st.r_idx, st.u5);
    rec.emratesPre = 1.0;                          // :1818
    rec.energiesPre = load_energy_row(HB, e_idx).energy;  // :1819
  }
  if (ballot64(alive)) {
    RayOut ro;
    if (!sampled) { st.u5 = 0.0; st.r_idx = 0; }
    phase_b<true, false, -1, false>(P, L, HB, A, st, e_idx >= 0 ? e_idx : 0, alive, ro, &rec);
  }
}

// The setup blob into the block's LDS copy, for the three kernels of kRecBlock threads
__device__ __forceinline__ void blob_to_lds(DevBlob& B, const DevBlob* __restrict__ blob) {
  const uint64_t* src = reinterpret_cast<const uint64_t*>(blob);
  uint64_t* dst = reinterpret_cast<uint64_t*>(&B);
  for (int i = threadIdx.x; i < (int)(sizeof(DevBlob) / 8); i += kRecBlock) dst[i] = src[i];
  __syncthreads();
}

__global__ __launch_bounds__(kRecBlock) void trace_records_kernel(HotA H, const DevBlob* __restrict__ blob, TraceArgs A,
                                                                   sart_axion_t* __restrict__ out, HotB HB,
                                                                   const double* __restrict__ uniforms) {
  __shared__ TablesLds S;
  __shared__ DevBlob B;
  blob_to_lds(B, blob);
  const DevParams& P = B.P;
  stage_tables<kRecBlock>(S, P, B.T);
  const LdsTables L{S.sincos, S.rcdf_hi, B.T.flux_radius_cdf, S.rguide, S.shells, S.lut};

  const uint64_t stride = (uint64_t)gridDim.x * kRecBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kRecBlock + threadIdx.x; i < A.n_rays; i += stride) {
    sart_axion_t rec = {};
    record_of_ray(H, P, L, HB, A, i, uniforms, rec);
    store_record(&out[i], rec);
  }
}

// Test twin of the radial verdict table (test entry sart_internal_radial_verdicts; no hot path reads it): the verdict byte of GIVEN
// radial distances by the table (radial_verdict_table, as stage A1 of the solar-source histogram kernels looks it up) and by the
// compares (radial_verdict_compares).  A ray's own radial distance cannot be placed to the last bit from its uniforms; here it can.
__global__ __launch_bounds__(256) void radial_verdict_kernel(HotA H, const DevBlob* __restrict__ blob, const double* __restrict__ radii, int n,
                                                             uint32_t* __restrict__ out_table, uint32_t* __restrict__ out_compares) {
  struct Lds {
    TablesLds S;
    RadialLds R;
    double behind[kRadialMarked + 1 - kRadialMax];   // (what a marked lane reads behind the table)
    DevBlob B;
  };
  __shared__ Lds lds;
  {
    const uint64_t* src = reinterpret_cast<const uint64_t*>(blob);
    uint64_t* dst = reinterpret_cast<uint64_t*>(&lds.B);
    for (int i = threadIdx.x; i < (int)(sizeof(DevBlob) / 8); i += 256) dst[i] = src[i];
    for (int i = threadIdx.x; i < kRadialMarked + 1 - kRadialMax; i += 256) lds.behind[i] = 0.0;
    __syncthreads();
  }
  const DevParams& P = lds.B.P;
  {
    const auto src = as_global(reinterpret_cast<const uint64_t*>(lds.B.T.shell_lut + kRadialTableOffset));
    uint64_t* dst = reinterpret_cast<uint64_t*>(&lds.R);
    for (int i = threadIdx.x; i < kRadialTableCells; i += 256) dst[i] = src[i];
  }
  stage_tables<256>(lds.S, P, lds.B.T, true);
  const LdsTables L{lds.S.sincos, lds.S.rcdf_hi, lds.B.T.flux_radius_cdf, lds.S.rguide, lds.S.shells, lds.S.lut, &lds.R, &lds.B.T};
  const bool cand_on = H.telescope_kind != SART_TK_LLNL;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const double radial = radii[i];
    out_table[i] = radial_verdict_table(H, P, L, cand_on, radial);
    out_compares[i] = radial_verdict_compares(H, P, L.shells, lds.B.T.shell_lut, cand_on, radial);
  }
}

// Diagnostic twin of the mirror-miss shortcut of trace_histogram_kernel (test entry sart_internal_mirror_miss; no hot path reads
// it): phase A of the record kernel for the launch's rays, then the shortcut's predicate beside phase B's own first-mirror
// arithmetic.  counts[0]: selected rays whose pick_root finds no root in the first mirror; [1]: those in a shell above the
// innermost; [2]: rays the predicate flags; [3]: flagged rays for which pick_root accepts a root; [4]: flagged rays whose nickel
// test is false ([3] and [4] are what the host's proofs exclude).
__global__ __launch_bounds__(kRecBlock) void mirror_miss_count_kernel(HotA H, const DevBlob* __restrict__ blob, TraceArgs A,
                                                                       unsigned long long* __restrict__ counts) {
  __shared__ TablesLds S;
  __shared__ DevBlob B;
  blob_to_lds(B, blob);
  const DevParams& P = B.P;
  stage_tables<kRecBlock>(S, P, B.T);
  const LdsTables L{S.sincos, S.rcdf_hi, B.T.flux_radius_cdf, S.rguide, S.shells, S.lut};
  uint32_t n[5] = {0, 0, 0, 0, 0};
  const uint64_t stride = (uint64_t)gridDim.x * kRecBlock;
  const uint64_t n_round = (A.n_rays + stride - 1) / stride * stride;   // whole waves run every pass (ballots)
  for (uint64_t i = (uint64_t)blockIdx.x * kRecBlock + threadIdx.x; i < n_round; i += stride) {
    RayState st;
    bool sampled, reached;
    double radial;
    LaneMasks masks;
    double r3sq;
    const uint64_t ray_id = A.ray_id_offset + i;
    const uint32_t u3_hi = word_of(stream_block(ray_id >> 2, A.seed_lo, A.seed_hi), (uint32_t)ray_id & 3u);
    const bool alive = phase_a<false, -1, false, false, false>(H, P, L, A.seed_lo, A.seed_hi, ray_id, u3_hi, st, sampled, reached, radial, masks, nullptr, &r3sq) &&
                       i < A.n_rays;
    const ShellDev& sh = L.shells[st.shell];
    const double X0 = st.X0, Y0 = st.Y0, tsx = st.tsx, tsy = st.tsy;
    const double Q0 = fma(X0, X0, Y0 * Y0), D0 = fma(X0, tsx, Y0 * tsy), A0 = fma(tsx, tsx, tsy * tsy);
    // phase B's first mirror and nickel test (phase_b), for a ray that missed
    double z1;
    uint64_t hit1_m;
    const bool hit1 = pick_root(A0 - sh.m1_k, D0 + sh.m1_hb, Q0 - sh.m1_cc, 0.0, sh.m1_zhi, z1, hit1_m);
    const double zcb = st.zcb;
    const double m1x = fma(zcb, tsx, X0), m1y = fma(zcb, tsy, Y0);
    const double n1z = normal_z_general(P, sh, 1, m1x, m1y, zcb);
    double wx = tsx, wy = tsy, wz = 1.0, sin_a1;
    const double sin2_a1 = reflect(wx, wy, wz, 1.0 + A0, m1x, m1y, n1z, fma(m1x, m1x, fma(m1y, m1y, n1z * n1z)), sin_a1);
    const double lz = P.l_mirror - zcb, num = sh.nickel_num;
    const bool nick = sin2_a1 * fma(lz, lz, num * num) > num * num;
    // the shortcut's predicate (run_phase_a of trace_histogram_kernel)
    const double zl = P.l_mirror, xe = fma(zl, tsx, X0), ye = fma(zl, tsy, Y0);
    const bool sure = alive & (radial > (double)P.mirror_miss_radius) & (fma(xe, xe, fma(ye, ye, kMirrorMissEps)) < r3sq) &
                      (A0 < (double)P.mirror_miss_slope_sq);
    n[0] += (uint32_t)(alive & !hit1);
    n[1] += (uint32_t)(alive & !hit1 & (st.shell > 0));
    n[2] += (uint32_t)sure;
    n[3] += (uint32_t)(sure & hit1);
    n[4] += (uint32_t)(sure & !nick);
  }
  for (int k = 0; k < 5; ++k)
    if (n[k]) atomicAdd(&counts[k], (unsigned long long)n[k]);
}

// ---- passed rays only (include/sart.h: sart_trace_records_passed): the records of one chunk, compacted in ray order ----------
// What generateResultPlots (raytracer.nim:2252-2283) and the scan sum (:2800) read of the record buffer: the records with
// `passed` set, and how many records have passedTillWindow / hitNickel set.  Three small kernels behind trace_records_kernel on
// the same stream: flags -> per-block counts, one-block exclusive scan, cooperative copy (each wave moves the records of its
// passed lanes as one contiguous run of 8-byte words: coalesced stores, 208-byte runs of loads).  Integer arithmetic only: the
// order and the counts do not depend on the launch geometry.
constexpr int kCompactBlock = 1024;                  // records per block of the three kernels
constexpr int kCompactMaxBlocks = 1024;              // blocks one scan covers: chunks of at most 2^20 records
__device__ __forceinline__ uint32_t record_flags(const sart_axion_t* rec, uint32_t i, uint32_t n) {
  return i < n ? *reinterpret_cast<const uint32_t*>(rec + i) : 0u;   // passed @0, passedTillWindow @1, hitNickel @2
}
// The flag word f of this thread's ray (0 behind the chunk's end) -> the passed rays of the block to block_counts[block], the
// other two flags of the block into counts[2] and counts[3]
__device__ __forceinline__ void count_flag_words(uint32_t f, uint32_t* __restrict__ block_counts,
                                                 unsigned long long* __restrict__ counts) {
  __shared__ uint32_t part[kCompactBlock / 64][3];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t np = (uint32_t)__popcll(ballot64((f & 0xFFu) != 0u)), nw = (uint32_t)__popcll(ballot64((f & 0xFF00u) != 0u)),
                 nn = (uint32_t)__popcll(ballot64((f & 0xFF0000u) != 0u));
  if (lane == 0) { part[wave][0] = np; part[wave][1] = nw; part[wave][2] = nn; }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t a = 0, b = 0, c = 0;
    for (int w = 0; w < kCompactBlock / 64; ++w) { a += part[w][0]; b += part[w][1]; c += part[w][2]; }
    block_counts[blockIdx.x] = a;
    if (b) atomicAdd(&counts[2], (unsigned long long)b);
    if (c) atomicAdd(&counts[3], (unsigned long long)c);
  }
}
__global__ __launch_bounds__(kCompactBlock) void records_count_kernel(const sart_axion_t* __restrict__ rec, uint32_t n,
                                                                       uint32_t* __restrict__ block_counts,
                                                                       unsigned long long* __restrict__ counts) {
  count_flag_words(record_flags(rec, blockIdx.x * kCompactBlock + threadIdx.x, n), block_counts, counts);
}
// block_counts[b] -> the index of block b's first passed record in the output (counts[1] = passed records of earlier chunks);
// counts[0] += n, counts[1] += the passed records of this chunk
__global__ __launch_bounds__(kCompactMaxBlocks) void records_scan_kernel(uint32_t* __restrict__ block_counts, uint32_t n_blocks,
                                                                          unsigned long long* __restrict__ block_first,
                                                                          unsigned long long* __restrict__ counts, uint32_t n) {
  __shared__ uint32_t wave_sum[kCompactMaxBlocks / 64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t v = threadIdx.x < n_blocks ? block_counts[threadIdx.x] : 0u;
  uint32_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64);
    if (lane >= d) incl += o;
  }
  if (lane == 63) wave_sum[wave] = incl;
  __syncthreads();
  uint32_t before = 0, total = 0;
  for (int w = 0; w < kCompactMaxBlocks / 64; ++w) { before += w < wave ? wave_sum[w] : 0u; total += wave_sum[w]; }
  const unsigned long long base = counts[1];
  if (threadIdx.x < n_blocks) block_first[threadIdx.x] = base + before + (incl - v);
  __syncthreads();   // every thread has read counts[1]
  if (threadIdx.x == 0) { counts[0] += n; counts[1] = base + total; }
}
__global__ __launch_bounds__(kCompactBlock) void records_scatter_kernel(const sart_axion_t* __restrict__ rec, uint32_t n,
                                                                         const unsigned long long* __restrict__ block_first,
                                                                         sart_axion_t* __restrict__ out, unsigned long long capacity) {
  __shared__ uint32_t wave_count[kCompactBlock / 64];
  __shared__ uint8_t src_lane[kCompactBlock / 64][64];
  const uint32_t i = blockIdx.x * kCompactBlock + threadIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool passed = (record_flags(rec, i, n) & 0xFFu) != 0u;
  const uint64_t m = ballot64(passed);
  const uint32_t cnt = (uint32_t)__popcll(m);
  const uint32_t prefix = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
  if (passed) src_lane[wave][prefix] = (uint8_t)lane;
  if (lane == 0) wave_count[wave] = cnt;
  __syncthreads();
  uint32_t before = 0;
  for (int w = 0; w < wave; ++w) before += wave_count[w];
  const unsigned long long first = block_first[blockIdx.x] + before;   // output index of this wave's first passed record
  constexpr uint32_t kWords = sizeof(sart_axion_t) / 8;                 // 26
  const uint64_t* src = reinterpret_cast<const uint64_t*>(rec + (blockIdx.x * kCompactBlock + wave * 64));
  uint64_t* dst = reinterpret_cast<uint64_t*>(out);
  for (uint32_t e = (uint32_t)lane; e < cnt * kWords; e += 64u) {
    const uint32_t r = e / kWords, w = e - r * kWords;
    if (first + r < capacity) dst[(first + r) * kWords + w] = src[(uint32_t)src_lane[wave][r] * kWords + w];
  }
}

// ---- passed rays as selected columns (include/sart.h: sart_trace_columns_passed) ---------------------------------------------
// The same rays, but only the words the caller selects (bit w of `mask` = word w of the record), structure-of-arrays.  Three
// steps per chunk of n rays: columns_stage_kernel traces the rays as trace_records_kernel does and writes, per ray, its flag
// word as u32 and each selected word into stage[slot][n] (slot = the number of selected words below it; coalesced 8-byte
// stores); columns_count_kernel counts the flags per block (records_scan_kernel then turns the counts into offsets, as for the
// records); columns_scatter_kernel moves the words of the passed rays to out[slot][capacity].
constexpr uint32_t kColumnWords = sizeof(sart_axion_t) / 8;   // 26; bit 26 of a mask = the ray id, which is computed, not staged
__global__ __launch_bounds__(kRecBlock) void columns_stage_kernel(HotA H, const DevBlob* __restrict__ blob, TraceArgs A,
                                                                   uint64_t* __restrict__ stage, uint32_t* __restrict__ flags,
                                                                   HotB HB, uint32_t mask) {
  __shared__ TablesLds S;
  __shared__ DevBlob B;
  blob_to_lds(B, blob);
  const DevParams& P = B.P;
  stage_tables<kRecBlock>(S, P, B.T);
  const LdsTables L{S.sincos, S.rcdf_hi, B.T.flux_radius_cdf, S.rguide, S.shells, S.lut};

  const uint64_t stride = (uint64_t)gridDim.x * kRecBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kRecBlock + threadIdx.x; i < A.n_rays; i += stride) {
    sart_axion_t rec = {};
    record_of_ray(H, P, L, HB, A, i, nullptr, rec);
    // the words of store_record, each behind a wave-uniform test of its mask bit (w is a literal in every call: the record is
    // never indexed at run time and stays in registers); the slot is a scalar popcount
    for_each_record_word(rec, [&](uint32_t w, uint64_t v) {
      if (w == 0u) flags[i] = (uint32_t)v;
      if ((mask >> w) & 1u) stage[(uint64_t)__popc(mask & ((1u << w) - 1u)) * A.n_rays + i] = v;
    });
  }
}
// records_count_kernel on the staged flag words
__global__ __launch_bounds__(kCompactBlock) void columns_count_kernel(const uint32_t* __restrict__ flags, uint32_t n,
                                                                       uint32_t* __restrict__ block_counts,
                                                                       unsigned long long* __restrict__ counts) {
  const uint32_t i = blockIdx.x * kCompactBlock + threadIdx.x;
  count_flag_words(i < n ? flags[i] : 0u, block_counts, counts);
}
// Passed ray i of the chunk goes to index d = block_first + (passed rays before it in its block) of every column, if d is below
// the capacity: column j of the output = out[j * capacity ..], the staged ones first, in mask order, then the ray id (bit 26).
__global__ __launch_bounds__(kCompactBlock) void columns_scatter_kernel(const uint64_t* __restrict__ stage, const uint32_t* __restrict__ flags,
                                                                         uint32_t n, const unsigned long long* __restrict__ block_first,
                                                                         uint64_t* __restrict__ out, unsigned long long capacity,
                                                                         uint32_t mask, unsigned long long ray_id0) {
  __shared__ uint32_t wave_count[kCompactBlock / 64];
  const uint32_t i = blockIdx.x * kCompactBlock + threadIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool passed = i < n && (flags[i] & 0xFFu) != 0u;
  const uint64_t m = ballot64(passed);
  const uint32_t prefix = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
  if (lane == 0) wave_count[wave] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t before = 0;
  for (int w = 0; w < wave; ++w) before += wave_count[w];
  const unsigned long long d = block_first[blockIdx.x] + before + prefix;
  if (!passed || d >= capacity) return;
  const uint32_t n_staged = (uint32_t)__popc(mask & ((1u << kColumnWords) - 1u));
  for (uint32_t j = 0; j < n_staged; ++j) out[(unsigned long long)j * capacity + d] = stage[(uint64_t)j * n + i];
  if ((mask >> kColumnWords) & 1u) out[(unsigned long long)n_staged * capacity + d] = ray_id0 + i;
}

// The offsets the kernels assume for their own arguments when they re-read them from the kernel-argument segment
// (reload_hot / reload_zones / reload_kernarg).  Not part of the C-ABI: tests/test_host_and_abi.py compares them with the
// argument offsets in the code object's metadata, so that a compiler that lays arguments out differently fails a CPU test
// instead of faulting on the GPU.
extern "C" __attribute__((visibility("default"))) void sart_internal_kernarg_layout(int32_t out[8]) {
  out[7] = (int32_t)sizeof(AScanKernArgs);   // (the angular-scan kernel: same offsets, its own last argument)
  out[0] = (int32_t)offsetof(HistKernArgs, H);
  out[1] = (int32_t)offsetof(HistKernArgs, blob);
  out[2] = (int32_t)offsetof(HistKernArgs, A);
  out[3] = (int32_t)offsetof(HistKernArgs, acc);
  out[4] = (int32_t)offsetof(HistKernArgs, HB);
  out[5] = (int32_t)offsetof(HistKernArgs, SC);
  out[6] = (int32_t)sizeof(HistKernArgs);
}

// ---- device math under test (tests/test_gpu_math.py): evaluates one helper on an array, not part of the C-ABI ----
__global__ void math_eval_kernel(int fn, const double* __restrict__ in, double* __restrict__ out, int n,
                                 const double* __restrict__ sincos_tab) {
  __shared__ double tab[2 * kSinCosEntries];
  for (int i = threadIdx.x; i < 2 * kSinCosEntries; i += blockDim.x) tab[i] = sincos_tab[i];
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x = in[i];
  double r = 0.0, sn, cs;
  const SinCosCoef K = sincos_coef();
  switch (fn) {
    case 0: r = frcp(x); break;
    case 1: r = frsq(x); break;
    case 2: r = fsqrt_pos(x); break;
    case 3: sincos_turns<2>(x, tab, K, &sn, &cs); r = sn; break;
    case 4: sincos_turns<2>(x, tab, K, &sn, &cs); r = cs; break;
    case 5: sincos_turns<1>(x, tab, K, &sn, &cs); r = sn; break;
    case 6: sincos_turns<1>(x, tab, K, &sn, &cs); r = cs; break;
    case 7: r = asin_small(x, x * x); break;
    case 8: r = cos_yaw_of_slope(x); break;
    case 9: r = atan_small(x); break;
    case 10: r = cos_small(x); break;
    case 11: r = fsqrt(x); break;
    case 12: r = exp_neg(x); break;
    case 13: r = cos_any(x, tab, K); break;
    case 14: r = cos_any_vvs(x, tab, GasCos::make()); break;
    // the paired forms (tests/test_gpu_horner_pairs.py): element i with its neighbour i ^ 1 as partner (n even), as the first
    // member (odd cases) or the second (even cases) of the pair - both must give the single form's bits for element i
    case 15: { const double y = in[min(i ^ 1, n - 1)]; double o; asin_small_pair(x, x * x, y, y * y, r, o); break; }
    case 16: { const double y = in[min(i ^ 1, n - 1)]; double o; asin_small_pair(y, y * y, x, x * x, o, r); break; }
    case 17: { double o; spoke_measure_pair(16, x, in[min(i ^ 1, n - 1)], r, o); break; }
    case 18: { double o; spoke_measure_pair(16, in[min(i ^ 1, n - 1)], x, o, r); break; }
    case 19: { double o; spoke_measure_pair(6, x, in[min(i ^ 1, n - 1)], r, o); break; }
    case 20: { double o; spoke_measure_pair(6, in[min(i ^ 1, n - 1)], x, o, r); break; }
    case 21: r = spoke_measure(16, x); break;
    case 22: r = spoke_measure(6, x); break;
    default: break;
  }
  out[i] = r;
}
extern "C" __attribute__((visibility("default"))) int sart_internal_math_eval(int fn, const double* in_host, double* out_host, int n,
                                                                               const double* sincos_table_host) {
  double *d_in = nullptr, *d_out = nullptr, *d_tab = nullptr;
  if (n < 1 || (fn >= 15 && fn <= 20 && (n & 1)) || hipMalloc(&d_in, (size_t)n * 8) != hipSuccess || hipMalloc(&d_out, (size_t)n * 8) != hipSuccess ||
      hipMalloc(&d_tab, 2 * kSinCosEntries * 8) != hipSuccess)
    return -1;
  (void)hipMemcpy(d_in, in_host, (size_t)n * 8, hipMemcpyHostToDevice);
  (void)hipMemcpy(d_tab, sincos_table_host, 2 * kSinCosEntries * 8, hipMemcpyHostToDevice);
  hipLaunchKernelGGL(math_eval_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, fn, d_in, d_out, n, d_tab);
  const hipError_t e = hipMemcpy(out_host, d_out, (size_t)n * 8, hipMemcpyDeviceToHost);
  (void)hipFree(d_in); (void)hipFree(d_out); (void)hipFree(d_tab);
  return e == hipSuccess ? 0 : -2;
}

// ---- the two CDF draws under test (tests/test_gpu_word_draw.py), not part of the C-ABI: the index of (row, word) from the
// word-exact form and from the general form, on a small table handed in from the host.  kind 0: energy draw, cdf = [n_rows][n_cols]
// (padded, turned into cdf_hi32 and given its guide here); kind 1: radius draw, cdf = [n_cols] staged into LDS by stage_tables.
void launch_cdf_hi32(const double* cdf_dev, uint32_t* out_dev, size_t n, hipStream_t stream);
void launch_build_guides(const double* ecdf_dev, int n_rows, int n_energies, uint16_t* eguide_dev, const double* rcdf_dev, int n_radii,
                         uint16_t* rguide_dev, uint32_t* status_dev, hipStream_t stream);
void launch_build_energy_records(const uint32_t* hi32_dev, const uint16_t* eguide_dev, int n_rows, int n_energies, uint32_t* records_dev,
                                 hipStream_t stream);
__global__ __launch_bounds__(256) void word_draw_energy_kernel(HotB HB, const int32_t* __restrict__ rows, const uint32_t* __restrict__ words, int n,
                                                               int32_t* __restrict__ out_word, int32_t* __restrict__ out_general) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t z = words[i];
  const double u = u52(z, 0u);
  out_word[i] = sample_energy_index<true>(HB, rows[i], u, z);
  out_general[i] = sample_energy_index<false>(HB, rows[i], u);
}
__global__ __launch_bounds__(256) void word_draw_radius_kernel(const double* __restrict__ rcdf, const uint16_t* __restrict__ rguide,
                                                               const double* __restrict__ sincos_tab, int n_radii,
                                                               const uint32_t* __restrict__ words, int n, int32_t* __restrict__ out_word,
                                                               int32_t* __restrict__ out_general) {
  __shared__ TablesLds S;
  DevParams P = {};
  P.n_radii = n_radii;       // (no shells, no look-up table: stage_tables copies none)
  DevTables T = {};
  T.sincos_tab = sincos_tab;
  T.flux_radius_cdf = rcdf;
  T.radius_guide = rguide;
  stage_tables<256>(S, P, T);
  const LdsTables L{S.sincos, S.rcdf_hi, rcdf, S.rguide, S.shells, S.lut};
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t z = words[i];
  out_word[i] = radius_draw<true>(L, z, u52(z, 0u));
  out_general[i] = radius_draw<false>(L, z, u52(z, 0u));
}
// use_records: the energy draw's word form goes through the bucket records where the table allows them (n_cols <= kEnergyRecordMaxEnergies);
// *records_used says whether it did, records_out (may be null) receives the table [n_rows][kEnergyGuideBuckets][4].
static int word_draw_impl(int kind, const double* cdf_host, int n_rows, int n_cols, const int32_t* rows_host, const uint32_t* words_host, int n,
                          int32_t* out_word_host, int32_t* out_general_host, bool use_records, int* records_used, uint32_t* records_out) {
  if (n < 1 || n_rows < 1 || n_cols < 1 || (kind != 0 && kind != 1) || (kind == 1 && (n_rows != 1 || n_cols > kMaxRadii)) || n_cols > 65535)
    return -1;
  if (kind == 0)
    for (int i = 0; i < n; ++i)
      if (rows_host[i] < 0 || rows_host[i] >= n_rows) return -1;
  const int stride = kind == 0 ? n_cols + kEnergyCdfPad : n_cols;
  std::vector<double> cdf((size_t)n_rows * stride, 1.0);
  for (int r = 0; r < n_rows; ++r)
    for (int k = 0; k < n_cols; ++k) cdf[(size_t)r * stride + k] = cdf_host[(size_t)r * n_cols + k];
  const size_t n_guide = kind == 0 ? (size_t)n_rows * kEnergyGuideEntries : (size_t)kRadiusGuideEntries;
  double *d_cdf = nullptr, *d_tab = nullptr;
  uint32_t *d_hi = nullptr, *d_words = nullptr, *d_status = nullptr;
  uint16_t* d_guide = nullptr;
  int32_t *d_rows = nullptr, *d_ow = nullptr, *d_og = nullptr;
  uint32_t* d_rec = nullptr;
  const bool records = use_records && kind == 0 && n_cols <= kEnergyRecordMaxEnergies;
  const size_t n_rec = (size_t)n_rows * kEnergyGuideBuckets * 4;
  if (records_used) *records_used = records ? 1 : 0;
  int rc = -2;
  if (records && hipMalloc(&d_rec, n_rec * 4) != hipSuccess) return rc;
  if (hipMalloc(&d_cdf, cdf.size() * 8) == hipSuccess && hipMalloc(&d_hi, cdf.size() * 4) == hipSuccess &&
      hipMalloc(&d_guide, n_guide * 2) == hipSuccess && hipMalloc(&d_words, (size_t)n * 4) == hipSuccess &&
      hipMalloc(&d_rows, (size_t)n * 4) == hipSuccess && hipMalloc(&d_ow, (size_t)n * 4) == hipSuccess &&
      hipMalloc(&d_og, (size_t)n * 4) == hipSuccess && hipMalloc(&d_status, 8) == hipSuccess &&
      hipMalloc(&d_tab, 2 * kSinCosEntries * 8) == hipSuccess) {
    (void)hipMemcpy(d_cdf, cdf.data(), cdf.size() * 8, hipMemcpyHostToDevice);
    (void)hipMemcpy(d_words, words_host, (size_t)n * 4, hipMemcpyHostToDevice);
    (void)hipMemset(d_rows, 0, (size_t)n * 4);
    (void)hipMemset(d_tab, 0, 2 * kSinCosEntries * 8);
    if (kind == 0) {
      (void)hipMemcpy(d_rows, rows_host, (size_t)n * 4, hipMemcpyHostToDevice);
      launch_cdf_hi32(d_cdf, d_hi, cdf.size(), nullptr);
      launch_build_guides(d_cdf, n_rows, n_cols, d_guide, nullptr, 0, nullptr, d_status, nullptr);
      HotB HB = {};
      HB.diff_flux_cdfs = d_cdf;
      HB.cdf_hi32 = d_hi;
      HB.energy_guide = d_guide;
      HB.n_energies = n_cols;
      HB.cdf_stride = stride;
      if (records) {
        launch_build_energy_records(d_hi, d_guide, n_rows, n_cols, d_rec, nullptr);
        HB.energy_records = d_rec;
        HB.records_on = 1;
      }
      hipLaunchKernelGGL(word_draw_energy_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, HB, d_rows, d_words, n, d_ow, d_og);
    } else {
      launch_build_guides(nullptr, 0, 0, nullptr, d_cdf, n_cols, d_guide, d_status, nullptr);
      hipLaunchKernelGGL(word_draw_radius_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, d_cdf, d_guide, d_tab, n_cols, d_words, n, d_ow,
                         d_og);
    }
    const hipError_t e1 = hipMemcpy(out_word_host, d_ow, (size_t)n * 4, hipMemcpyDeviceToHost);
    const hipError_t e2 = hipMemcpy(out_general_host, d_og, (size_t)n * 4, hipMemcpyDeviceToHost);
    const hipError_t e3 = (records && records_out) ? hipMemcpy(records_out, d_rec, n_rec * 4, hipMemcpyDeviceToHost) : hipSuccess;
    rc = (e1 == hipSuccess && e2 == hipSuccess && e3 == hipSuccess && hipGetLastError() == hipSuccess) ? 0 : -2;
  }
  (void)hipFree(d_cdf); (void)hipFree(d_hi); (void)hipFree(d_guide); (void)hipFree(d_words); (void)hipFree(d_rows);
  (void)hipFree(d_ow); (void)hipFree(d_og); (void)hipFree(d_status); (void)hipFree(d_tab); (void)hipFree(d_rec);
  return rc;
}
extern "C" __attribute__((visibility("default"))) int sart_internal_word_draw(int kind, const double* cdf_host, int n_rows, int n_cols,
                                                                               const int32_t* rows_host, const uint32_t* words_host, int n,
                                                                               int32_t* out_word_host, int32_t* out_general_host) {
  return word_draw_impl(kind, cdf_host, n_rows, n_cols, rows_host, words_host, n, out_word_host, out_general_host, true, nullptr, nullptr);
}
// The energy draw alone (tests/test_gpu_energy_records.py), with the bucket records (use_records != 0, where the table allows them:
// *records_used) or in two levels; records_out may be null.
extern "C" __attribute__((visibility("default"))) int sart_internal_record_draw(const double* cdf_host, int n_rows, int n_cols,
                                                                                 const int32_t* rows_host, const uint32_t* words_host, int n,
                                                                                 int use_records, int32_t* out_word_host, int32_t* out_general_host,
                                                                                 int* records_used, uint32_t* records_out) {
  return word_draw_impl(0, cdf_host, n_rows, n_cols, rows_host, words_host, n, out_word_host, out_general_host, use_records != 0, records_used,
                        records_out);
}

// ---- launch wrappers (called from sart_api.hip) ----
int records_block() { return kRecBlock; }
// Variants: 0 = specialised (solar source, no hole loop) vacuum, not rotated; 1 = generic, not rotated; 2 = generic, rotated;
// 3 = specialised, gas stage; 4 = specialised, rotated; 5 = variant 0 with the constant path in the magnetic field (PATHC);
// 6 = variant 3 with the constant path; 7 / 8 = 5 / 6 with their wave-uniform switches folded (folded_histogram_kernel; the host
// picks them per launch: sart_device.h, folded_form_applies).  All with 1024 threads = 4 waves / SIMD (measured fastest of 256 / 512 / 768 / 1024).
// The fused mass scan exists for the variants that can run the gas stage: 1, 2, 3, 6.
int histogram_block_of(int) { return 1024; }

#define SART_HIST_VARIANTS(X) \
  X(0, true, false, 0, false) X(1, false, false, -1, false) X(2, false, true, -1, false) X(3, true, false, 1, false) \
  X(4, true, true, 0, false) X(5, true, false, 0, true) X(6, true, false, 1, true)
// 7 / 8: the folded forms of 5 / 6 (folded_histogram_kernel<1024, GAS, FIXED>; launch only: grid and occupancy are those of 5 / 6)
#define SART_HIST_FOLDED_VARIANTS(X) X(7, 0) X(8, 1)
#define SART_SCAN_VARIANTS(X) X(1, false, false, -1, false) X(2, false, true, -1, false) X(3, true, false, 1, false) X(6, true, false, 1, true)

// The instantiation of fold kernel K for the accumulation mode
#define SART_FOLD_OF(K, fixed) ((fixed) ? K<true> : K<false>)
// What every accumulator launch ends with: the scalars (acc scalars += the workgroup partials) ...
static void launch_scalars_fold(double* scalars, const double* partials, const TraceArgs& A, int n_blocks, hipStream_t stream, bool fixed) {
  if (fixed)
    hipLaunchKernelGGL(fold_scalars_fixed_kernel, dim3(1), dim3(256), 0, stream, reinterpret_cast<long long*>(scalars),
                       reinterpret_cast<const long long*>(partials), n_blocks, (long long)A.n_rays);
  else
    hipLaunchKernelGGL(fold_scalars_kernel, dim3(1), dim3(256), 0, stream, scalars, partials, n_blocks, (double)A.n_rays);
}
// ... and, where the launch used image replicas, those
static void launch_accumulator_folds(const TraceArgs& A, double* acc, int n_blocks, hipStream_t stream, bool fixed) {
  const int n_img = A.image_nx * A.image_ny;
  launch_scalars_fold(acc + n_img, A.partials, A, n_blocks, stream, fixed);
  if (A.replica_mask == 0u) return;
  const dim3 grid((n_img + 255) / 256);
  if (fixed)
    hipLaunchKernelGGL(fold_replicas_kernel<long long>, grid, dim3(256), 0, stream, reinterpret_cast<long long*>(acc),
                       reinterpret_cast<long long*>(A.replicas), n_img, (int)A.replica_mask + 1, A.replica_stride);
  else
    hipLaunchKernelGGL(fold_replicas_kernel<double>, grid, dim3(256), 0, stream, acc, A.replicas, n_img, (int)A.replica_mask + 1, A.replica_stride);
}

int histogram_blocks_per_cu(int variant) {   // the FIXED64 and SCAN instantiations use the same LDS and launch bounds
  int n = 0;
  hipError_t e = hipErrorInvalidValue;
  switch (variant) {
#define X(ID, F, R, G, PC) case ID: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, trace_histogram_kernel<1024, F, R, G, PC, false>, 1024, 0); break;
    SART_HIST_VARIANTS(X)
#undef X
    default: break;
  }
  return (e == hipSuccess && n > 0) ? n : 1;
}

void launch_trace_histogram(const HotA& H, const HotB& HB, const DevBlob* blob, const TraceArgs& A, double* acc, int n_blocks,
                            hipStream_t stream, int variant, bool fixed) {
  ScanArgs SC;
  memset(&SC, 0, sizeof SC);   // n_masses = 0: not a scan
  switch (variant + (fixed ? 100 : 0)) {
#define X(ID, F, R, G, PC) \
    case ID: hipLaunchKernelGGL((trace_histogram_kernel<1024, F, R, G, PC, false>), dim3(n_blocks), dim3(1024), 0, stream, H, blob, A, acc, HB, SC); break; \
    case 100 + ID: hipLaunchKernelGGL((trace_histogram_kernel<1024, F, R, G, PC, true>), dim3(n_blocks), dim3(1024), 0, stream, H, blob, A, acc, HB, SC); break;
    SART_HIST_VARIANTS(X)
#undef X
#define X(ID, G) \
    case ID: hipLaunchKernelGGL((folded_histogram_kernel<1024, G, false>), dim3(n_blocks), dim3(1024), 0, stream, H, blob, A, acc, HB, SC); break; \
    case 100 + ID: hipLaunchKernelGGL((folded_histogram_kernel<1024, G, true>), dim3(n_blocks), dim3(1024), 0, stream, H, blob, A, acc, HB, SC); break;
    SART_HIST_FOLDED_VARIANTS(X)
#undef X
    default: return;
  }
  launch_accumulator_folds(A, acc, n_blocks, stream, fixed);
}

// One group of SC.n_masses <= kScanMaxMasses masses over the rays of A: trace + per-mass accumulation, then the fold into
// `rows` (the group's first row of the scan accumulator) and, if `shared_row`, into the scan's counter row.
bool launch_trace_mass_scan(const HotA& H, const HotB& HB, const DevBlob* blob, const TraceArgs& A, const ScanArgs& SC, double* rows,
                            double* shared_row, int n_blocks, hipStream_t stream, int variant, bool fixed) {
  double* const no_acc = nullptr;   // a scan accumulates no image and no spectra
  switch (variant + (fixed ? 100 : 0)) {
#define X(ID, F, R, G, PC) \
    case ID: hipLaunchKernelGGL((trace_histogram_kernel<1024, F, R, G, PC, false, true>), dim3(n_blocks), dim3(1024), 0, stream, H, blob, A, no_acc, HB, SC); break; \
    case 100 + ID: hipLaunchKernelGGL((trace_histogram_kernel<1024, F, R, G, PC, true, true>), dim3(n_blocks), dim3(1024), 0, stream, H, blob, A, no_acc, HB, SC); break;
    SART_SCAN_VARIANTS(X)
#undef X
    default: return false;
  }
  hipLaunchKernelGGL(SART_FOLD_OF(fold_scan_kernel, fixed), dim3(1), dim3(1024), 0, stream, rows, shared_row, A.partials, SC.partials, n_blocks,
                     SC.n_masses, (double)A.n_rays);
  return true;
}

// The banded form of the same group (SC.n_bands bands): the scan rows as above, and the band cells into `block0` (the block of the
// group's first mass in the spectra accumulator) and, if `counts` (with `shared_row`), the per-band counts into the counts block.
int mass_scan_spectra_blocks_per_cu(int variant) {
  int n = 0;
  hipError_t e = hipErrorInvalidValue;
  switch (variant) {
#define X(ID, F, R, G, PC) case ID: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, mass_scan_spectra_kernel<1024, F, R, G, PC, false>, 1024, 0); break;
    SART_SCAN_VARIANTS(X)
#undef X
    default: break;
  }
  return (e == hipSuccess && n > 0) ? n : 1;
}
bool launch_trace_mass_scan_spectra(const HotA& H, const HotB& HB, const DevBlob* blob, const TraceArgs& A, const ScanArgs& SC, double* rows,
                                    double* shared_row, double* block0, double* counts, int n_blocks, hipStream_t stream, int variant, bool fixed) {
  double* const no_acc = nullptr;
  switch (variant + (fixed ? 100 : 0)) {
#define X(ID, F, R, G, PC) \
    case ID: hipLaunchKernelGGL((mass_scan_spectra_kernel<1024, F, R, G, PC, false>), dim3(n_blocks), dim3(1024), 0, stream, H, blob, A, no_acc, HB, SC); break; \
    case 100 + ID: hipLaunchKernelGGL((mass_scan_spectra_kernel<1024, F, R, G, PC, true>), dim3(n_blocks), dim3(1024), 0, stream, H, blob, A, no_acc, HB, SC); break;
    SART_SCAN_VARIANTS(X)
#undef X
    default: return false;
  }
  const dim3 grid(SC.n_masses + (counts ? 1 : 0));
  const double* const band_partials = SC.partials + (size_t)n_blocks * (kScanMaxMasses * kScanPartialSlots);   // behind the plain rows
  hipLaunchKernelGGL(SART_FOLD_OF(fold_scan_kernel, fixed), dim3(1), dim3(1024), 0, stream, rows, shared_row, A.partials, SC.partials, n_blocks,
                     SC.n_masses, (double)A.n_rays);
  hipLaunchKernelGGL(SART_FOLD_OF(fold_scan_bands_kernel, fixed), grid, dim3(1024), 0, stream, block0, counts, band_partials, n_blocks, SC.n_masses,
                     SC.n_bands + 1);
  return true;
}

// One group of AN.n_angles <= kAScanMaxAngles telescope angles over the rays of A: trace + per-angle accumulation, then the fold
// into `rows` (the group's first row of the scan accumulator) and, if `shared_row`, into the scan's counter row.  `fast`: the
// specialised instantiation (solar source, no hole loop, vacuum), else the one that reads those switches at run time.  `images`:
// the image scan, and behind the rows the scalars of every angle's block (A.replicas + k A.replica_stride) from
// img_partials[k][n_blocks][SART_ACC_COUNT]; without it img_partials is null.
static void (*const kAScanKernels[2][2][2])(HotA, const DevBlob*, TraceArgs, double*, HotB, AScanArgs) = {   // [images][fast][fixed]
    {{trace_angular_scan_kernel<1024, false, -1, false>, trace_angular_scan_kernel<1024, false, -1, true>},
     {trace_angular_scan_kernel<1024, true, 0, false>, trace_angular_scan_kernel<1024, true, 0, true>}},
    {{ascan_images_kernel<1024, false, -1, false>, ascan_images_kernel<1024, false, -1, true>},
     {ascan_images_kernel<1024, true, 0, false>, ascan_images_kernel<1024, true, 0, true>}}};
int angular_scan_blocks_per_cu(bool images, bool fast) {
  int n = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kAScanKernels[images][fast][0], 1024, 0);
  return (e == hipSuccess && n > 0) ? n : 1;
}
void launch_trace_angular_scan(const HotA& H, const HotB& HB, const DevBlob* blob, const TraceArgs& A, const AScanArgs& AN, double* img_partials,
                               double* rows, double* shared_row, int n_blocks, hipStream_t stream, bool images, bool fast, bool fixed) {
  hipLaunchKernelGGL(kAScanKernels[images][fast][fixed], dim3(n_blocks), dim3(1024), 0, stream, H, blob, A, img_partials, HB, AN);
  hipLaunchKernelGGL(SART_FOLD_OF(fold_ascan_kernel, fixed), dim3(1), dim3(1024), 0, stream, rows, shared_row, AN.partials, n_blocks, AN.n_angles,
                     (double)A.n_rays);
  if (!images) return;
  const size_t n_img = (size_t)A.image_nx * (size_t)A.image_ny;
  for (int k = 0; k < AN.n_angles; ++k)
    launch_scalars_fold(A.replicas + (size_t)k * A.replica_stride + n_img, img_partials + (size_t)k * (size_t)n_blocks * SART_ACC_COUNT, A, n_blocks,
                        stream, fixed);
}

// The fused energy scan of one launch group: the kernel (generic variants: `rotated` = hist_variant_of 2), then the fold into
// `rows` (the group's first row of the scan accumulator) and, if `shared_row`, into the scan's counter row.
int energy_scan_blocks_per_cu(bool rotated) {
  int n = 0;
  const hipError_t e = rotated ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, energy_scan_kernel<1024, true, false>, 1024, 0)
                               : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, energy_scan_kernel<1024, false, false>, 1024, 0);
  return (e == hipSuccess && n > 0) ? n : 1;
}
void launch_trace_energy_scan(const HotA& H, const HotB& HB, const DevBlob* blob, const TraceArgs& A, const EScanArgs& EN, double* rows,
                              double* shared_row, int n_blocks, hipStream_t stream, bool rotated, bool fixed) {
  double* const no_acc = nullptr;
  switch ((rotated ? 2 : 0) + (fixed ? 1 : 0)) {
    case 0: hipLaunchKernelGGL((energy_scan_kernel<1024, false, false>), dim3(n_blocks), dim3(1024), 0, stream, H, blob, A, no_acc, HB, EN); break;
    case 1: hipLaunchKernelGGL((energy_scan_kernel<1024, false, true>), dim3(n_blocks), dim3(1024), 0, stream, H, blob, A, no_acc, HB, EN); break;
    case 2: hipLaunchKernelGGL((energy_scan_kernel<1024, true, false>), dim3(n_blocks), dim3(1024), 0, stream, H, blob, A, no_acc, HB, EN); break;
    default: hipLaunchKernelGGL((energy_scan_kernel<1024, true, true>), dim3(n_blocks), dim3(1024), 0, stream, H, blob, A, no_acc, HB, EN); break;
  }
  hipLaunchKernelGGL(SART_FOLD_OF(fold_escan_kernel, fixed), dim3(1), dim3(1024), 0, stream, rows, shared_row, A.partials, EN.partials, n_blocks,
                     EN.n_energies, (double)A.n_rays);
}

// The breakdown launches (generic variants: `rotated` = hist_variant_of 2): the kernel, then the folds of launch_trace_histogram
// (scalars, replicas) and the fold of the breakdown's table - one workgroup per row: shell or channel - into the caller's block.
template <class Args>
struct BreakdownKernels {
  void (*trace[4])(HotA, const DevBlob*, TraceArgs, double*, HotB, Args);   // [kernel_index(rotated, fixed)]
  void (*fold[2])(double*, const double*, int);                             // [fixed ? 0 : 1]
};
// (the instantiations stand in the order in which the code object has always held them: <ROT, FIXED> = <1, 0>, <0, 0>, <0, 1>, <1, 1>)
static int kernel_index(bool rotated, bool fixed) { return fixed ? (rotated ? 3 : 2) : (rotated ? 0 : 1); }
static const BreakdownKernels<ShellArgs> kShellKernels = {
    {shell_histogram_kernel<1024, true, false>, shell_histogram_kernel<1024, false, false>, shell_histogram_kernel<1024, false, true>,
     shell_histogram_kernel<1024, true, true>},
    {fold_shells_kernel<true>, fold_shells_kernel<false>}};
static const BreakdownKernels<ChannelArgs> kChannelKernels = {
    {channel_histogram_kernel<1024, true, false>, channel_histogram_kernel<1024, false, false>,
     channel_histogram_kernel<1024, false, true>, channel_histogram_kernel<1024, true, true>},
    {fold_channels_kernel<true>, fold_channels_kernel<false>}};
static const BreakdownKernels<OriginArgs> kOriginKernels = {
    {origin_histogram_kernel<1024, true, false>, origin_histogram_kernel<1024, false, false>,
     origin_histogram_kernel<1024, false, true>, origin_histogram_kernel<1024, true, true>},
    {fold_origin_kernel<true>, fold_origin_kernel<false>}};
static const BreakdownKernels<ApertureArgs> kApertureKernels = {
    {aperture_histogram_kernel<1024, true, false>, aperture_histogram_kernel<1024, false, false>,
     aperture_histogram_kernel<1024, false, true>, aperture_histogram_kernel<1024, true, true>},
    {fold_origin_kernel<true>, fold_origin_kernel<false>}};   // (the head is the origin block's)

template <class Args>
static int breakdown_blocks_per_cu(const BreakdownKernels<Args>& K, bool rotated) {
  int n = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, K.trace[kernel_index(rotated, false)], 1024, 0);
  return (e == hipSuccess && n > 0) ? n : 1;
}
template <class Args>
static void launch_breakdown_histogram(const BreakdownKernels<Args>& K, const HotA& H, const HotB& HB, const DevBlob* blob,
                                       const TraceArgs& A, double* acc, const Args& BD, int n_rows, int n_blocks, hipStream_t stream,
                                       bool rotated, bool fixed) {
  hipLaunchKernelGGL(K.trace[kernel_index(rotated, fixed)], dim3(n_blocks), dim3(1024), 0, stream, H, blob, A, acc, HB, BD);
  launch_accumulator_folds(A, acc, n_blocks, stream, fixed);
  hipLaunchKernelGGL(K.fold[fixed ? 0 : 1], dim3(n_rows), dim3(64), 0, stream, BD.block, BD.partials, n_blocks);
}
int shell_histogram_blocks_per_cu(bool rotated) { return breakdown_blocks_per_cu(kShellKernels, rotated); }
int channel_histogram_blocks_per_cu(bool rotated) { return breakdown_blocks_per_cu(kChannelKernels, rotated); }
void launch_shell_histogram(const HotA& H, const HotB& HB, const DevBlob* blob, const TraceArgs& A, double* acc, const ShellArgs& SH,
                            int n_blocks, hipStream_t stream, bool rotated, bool fixed) {
  launch_breakdown_histogram(kShellKernels, H, HB, blob, A, acc, SH, SH.n_shells, n_blocks, stream, rotated, fixed);
}
void launch_channel_histogram(const HotA& H, const HotB& HB, const DevBlob* blob, const TraceArgs& A, double* acc, const ChannelArgs& CH,
                              int n_blocks, hipStream_t stream, bool rotated, bool fixed) {
  launch_breakdown_histogram(kChannelKernels, H, HB, blob, A, acc, CH, CH.n_channels, n_blocks, stream, rotated, fixed);
}
int origin_histogram_blocks_per_cu(bool rotated) { return breakdown_blocks_per_cu(kOriginKernels, rotated); }
void launch_origin_histogram(const HotA& H, const HotB& HB, const DevBlob* blob, const TraceArgs& A, double* acc, const OriginArgs& OG,
                             int n_blocks, hipStream_t stream, bool rotated, bool fixed) {
  launch_breakdown_histogram(kOriginKernels, H, HB, blob, A, acc, OG, 1, n_blocks, stream, rotated, fixed);   // (one row: the head)
}
int aperture_histogram_blocks_per_cu(bool rotated) { return breakdown_blocks_per_cu(kApertureKernels, rotated); }
void launch_aperture_histogram(const HotA& H, const HotB& HB, const DevBlob* blob, const TraceArgs& A, double* acc, const ApertureArgs& AP,
                               int n_blocks, hipStream_t stream, bool rotated, bool fixed) {
  launch_breakdown_histogram(kApertureKernels, H, HB, blob, A, acc, AP, 1, n_blocks, stream, rotated, fixed);   // (one row: the head)
}
void launch_finalize_origin(const void* in, double* out, size_t n_cells, double q_w, double q_w2, void* check_dev, hipStream_t stream) {
  FinalizeOriginArgs F{(long long)n_cells, q_w, q_w2};
  FixedCheck* const C = static_cast<FixedCheck*>(check_dev);
  (void)hipMemsetAsync(reinterpret_cast<char*>(C) + 8, 0, offsetof(FixedCheck, fail) - 8, stream);   // everything but the status word and the failure record
  const unsigned n_blocks = (unsigned)std::min<size_t>((n_cells + 255) / 256, 2048);
  if (n_blocks > 0)
    hipLaunchKernelGGL(finalize_origin_kernel, dim3(n_blocks), dim3(256), 0, stream, reinterpret_cast<const long long*>(in), out, F, C);
  hipLaunchKernelGGL(finalize_origin_head_kernel, dim3(1), dim3(64), 0, stream, reinterpret_cast<const long long*>(in), out, F, C);
}
void launch_finalize_shells(const void* in, double* out, int n_shells, int n_energies1, int spectra, double q_w, double q_w2,
                            void* check_dev, hipStream_t stream) {
  FinalizeShellsArgs F{n_shells, n_energies1, spectra, 0, q_w, q_w2};
  hipLaunchKernelGGL(finalize_shells_kernel, dim3(n_shells), dim3(256), 0, stream, reinterpret_cast<const long long*>(in), out, F,
                     static_cast<FixedCheck*>(check_dev));
}

void launch_finalize_channels(const void* in, double* out, int n_channels, int n_energies1, int spectra, size_t n_img, double q_w,
                              double q_w2, void* check_dev, hipStream_t stream) {
  FinalizeChannelsArgs F{n_channels, n_energies1, spectra, 0, (long long)n_img, q_w, q_w2};
  hipLaunchKernelGGL(finalize_channels_kernel, dim3(n_channels), dim3(256), 0, stream, reinterpret_cast<const long long*>(in), out, F,
                     static_cast<FixedCheck*>(check_dev));
}
// first_bad_dev: one 8-byte word, set to ~0 here
void launch_channel_fractions(const double* rates_dev, const double* total_dev, double* frac_dev, int n_channels, int stride,
                              size_t n_cells, unsigned long long* first_bad_dev, hipStream_t stream) {
  (void)hipMemsetAsync(first_bad_dev, 0xFF, sizeof(unsigned long long), stream);
  hipLaunchKernelGGL(channel_fractions_kernel, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), 0, stream, rates_dev, total_dev,
                     frac_dev, n_channels, stride, (long long)n_cells, first_bad_dev);
}

size_t fixed_check_bytes() { return sizeof(FixedCheck); }
// "pixels 123 + 456 x 2^40 quanta, wanted ..." from a host copy of the context's FixedCheck (the error message of a failed
// conservation check, sart_api.hip: status_take)
std::string fixed_check_describe(const void* host_copy) {
  const FixedCheck& C = *static_cast<const FixedCheck*>(host_copy);
  const char* names[5] = {"pixels", "SUM_WEIGHTS - outside", "radial bins", "energy bins", "SUM_WEIGHTS"};
  std::string s = " [quanta as lo + hi x 2^40:";
  for (int i = 0; i < 5; ++i) {
    if ((i == 2 || i == 3) && !C.spectra) continue;
    long long lo = C.fail[2 * i], hi = C.fail[2 * i + 1];
    limbs_normalise(lo, hi);
    s += std::string(i ? "," : "") + " " + names[i] + " " + std::to_string(lo) + " + " + std::to_string(hi);
  }
  return s + "]";
}
void launch_rollover_fixed(void* acc, void* hi, size_t n, void* check_dev, hipStream_t stream) {
  hipLaunchKernelGGL(rollover_fixed_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, static_cast<long long*>(acc),
                     static_cast<long long*>(hi), (long long)n, static_cast<FixedCheck*>(check_dev));
}
void launch_finalize_fixed(const void* in, const void* hi, double* out, size_t n_img, int spectra, int n_radial_bins, int n_energies1, double q_w,
                           double q_w2, double q_pos, double q_refl, void* check_dev, hipStream_t stream) {
  FinalizeArgs F{(long long)n_img, spectra, n_radial_bins, n_energies1, 0, q_w, q_w2, q_pos, q_refl};
  const size_t total = n_img + SART_ACC_COUNT + (spectra ? 2 * (size_t)n_radial_bins + 3 * (size_t)n_energies1 : 0);
  FixedCheck* const C = static_cast<FixedCheck*>(check_dev);
  (void)hipMemsetAsync(reinterpret_cast<char*>(C) + 8, 0, offsetof(FixedCheck, fail) - 8, stream);   // everything but the status word and the failure record
  hipLaunchKernelGGL(finalize_fixed_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream,
                     reinterpret_cast<const long long*>(in), reinterpret_cast<const long long*>(hi), out, F, C);
  hipLaunchKernelGGL(fixed_check_kernel, dim3(1), dim3(1), 0, stream, C);
}
// rows [0, n_masses) of in / out with the quanta q_w[k], q_w2[k]; shared_row >= 0: that row (relative to `in`) holds the counters
void launch_finalize_scan(const void* in, double* out, int n_masses, const double* q_w, const double* q_w2, int shared_row,
                          void* check_dev, hipStream_t stream, uint32_t counter_slots) {
  FinalizeScanArgs F;
  memset(&F, 0, sizeof F);
  F.n_masses = n_masses;
  F.shared_row = shared_row;
  F.counter_slots = counter_slots;
  for (int k = 0; k < n_masses; ++k) { F.q_w[k] = q_w[k]; F.q_w2[k] = q_w2[k]; }
  hipLaunchKernelGGL(finalize_scan_kernel, dim3(1), dim3(64), 0, stream, reinterpret_cast<const long long*>(in), out, F, static_cast<FixedCheck*>(check_dev));
}
// The spectra blocks [0, n_masses) of in / out (a group of masses, quanta q_w[k], q_w2[k]) against the group's RAW scan rows;
// counts_in: the counts block is converted too and held to `shared_row` (the raw counter row of the scan).
void launch_finalize_scan_bands(const void* rows, const void* shared_row, const void* in, double* out, const void* counts_in, double* counts_out,
                                int n_masses, int n_cells, const double* q_w, const double* q_w2, void* check_dev, hipStream_t stream) {
  FinalizeBandsArgs F;
  memset(&F, 0, sizeof F);
  F.n_masses = n_masses;
  F.n_cells = n_cells;
  for (int k = 0; k < n_masses; ++k) { F.q_w[k] = q_w[k]; F.q_w2[k] = q_w2[k]; }
  hipLaunchKernelGGL(finalize_scan_bands_kernel, dim3(n_masses + (counts_in ? 1 : 0)), dim3(64), 0, stream, static_cast<const long long*>(rows),
                     static_cast<const long long*>(shared_row), static_cast<const long long*>(in), out, static_cast<const long long*>(counts_in),
                     counts_out, F, static_cast<FixedCheck*>(check_dev));
}
int compact_chunk_max() { return kCompactBlock * kCompactMaxBlocks; }
// scratch: block_counts[kCompactMaxBlocks] u32, block_first[kCompactMaxBlocks] u64; counts[4] = {n_rays, n_passed, n_passed_till_window, n_hit_nickel}
void launch_compact_records(const sart_axion_t* rec, uint32_t n, sart_axion_t* out, unsigned long long capacity, uint32_t* block_counts,
                            unsigned long long* block_first, unsigned long long* counts, hipStream_t stream) {
  const uint32_t n_blocks = (n + kCompactBlock - 1) / kCompactBlock;
  hipLaunchKernelGGL(records_count_kernel, dim3(n_blocks), dim3(kCompactBlock), 0, stream, rec, n, block_counts, counts);
  hipLaunchKernelGGL(records_scan_kernel, dim3(1), dim3(kCompactMaxBlocks), 0, stream, block_counts, n_blocks, block_first, counts, n);
  hipLaunchKernelGGL(records_scatter_kernel, dim3(n_blocks), dim3(kCompactBlock), 0, stream, rec, n, block_first, out, capacity);
}
void launch_trace_records(const HotA& H, const HotB& HB, const DevBlob* blob, const TraceArgs& A, sart_axion_t* out, int n_blocks,
                          hipStream_t stream, const double* uniforms_dev) {
  hipLaunchKernelGGL(trace_records_kernel, dim3(n_blocks), dim3(kRecBlock), 0, stream, H, blob, A, out, HB, uniforms_dev);
}
// counts: [5], zeroed by the caller
void launch_mirror_miss_count(const HotA& H, const DevBlob* blob, const TraceArgs& A, unsigned long long* counts, int n_blocks, hipStream_t stream) {
  hipLaunchKernelGGL(mirror_miss_count_kernel, dim3(n_blocks), dim3(kRecBlock), 0, stream, H, blob, A, counts);
}
// out_table[n], out_compares[n]: the verdict byte of radii[i] by either form (cand_on as trace_histogram_kernel's unrotated
// instantiations have it).  H.radial_table must be set.
void launch_radial_verdicts(const HotA& H, const DevBlob* blob, const double* radii, int n, uint32_t* out_table, uint32_t* out_compares,
                            hipStream_t stream) {
  hipLaunchKernelGGL(radial_verdict_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, H, blob, radii, n, out_table, out_compares);
}
// stage: [popcount(mask & 0x3FFFFFF)][A.n_rays] words, flags: [A.n_rays]
void launch_stage_columns(const HotA& H, const HotB& HB, const DevBlob* blob, const TraceArgs& A, uint64_t* stage, uint32_t* flags,
                          uint32_t mask, int n_blocks, hipStream_t stream) {
  hipLaunchKernelGGL(columns_stage_kernel, dim3(n_blocks), dim3(kRecBlock), 0, stream, H, blob, A, stage, flags, HB, mask);
}
// scratch and counts as in launch_compact_records; out: [popcount(mask)][capacity] words
void launch_compact_columns(const uint64_t* stage, const uint32_t* flags, uint32_t n, uint32_t mask, unsigned long long ray_id0, uint64_t* out,
                            unsigned long long capacity, uint32_t* block_counts, unsigned long long* block_first,
                            unsigned long long* counts, hipStream_t stream) {
  const uint32_t n_blocks = (n + kCompactBlock - 1) / kCompactBlock;
  hipLaunchKernelGGL(columns_count_kernel, dim3(n_blocks), dim3(kCompactBlock), 0, stream, flags, n, block_counts, counts);
  hipLaunchKernelGGL(records_scan_kernel, dim3(1), dim3(kCompactMaxBlocks), 0, stream, block_counts, n_blocks, block_first, counts, n);
  hipLaunchKernelGGL(columns_scatter_kernel, dim3(n_blocks), dim3(kCompactBlock), 0, stream, stage, flags, n, block_first, out, capacity, mask,
                     ray_id0);
}

}  // namespace sart
