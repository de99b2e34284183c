// The body of trace_histogram_kernel and of mass_scan_spectra_kernel (sart_kernels.hip, which describes it and includes this file
// once inside each of the two: one text, so that the histogram kernels compile to the code they had as a single kernel - a shared
// __device__ function, inlined, does not).  In scope: the template parameters BLOCK, FAST, ROT, GAS, PATHC, FIXED, the constants SCAN
// and BANDS, the configuration type CFG (sart_kernels.hip: HistCfg - RunTimeCfg, or FoldedCfg in folded_histogram_kernel), and the
// kernel's parameters H, blob, A, acc, HBarg, SCarg.
  // One LDS object with the tables FIRST: their addresses then fit the 16-bit offset field of the ds_ instructions, and a
  // lookup is `ds_read v, v_index_scaled offset:TABLE` instead of a literal moved into a register and added to the index
  // (the rings are addressed from a per-wave scalar base anyway).
  struct LdsLayout {
    TablesLds S;
    RadialLds R;                          // (in front of the tile: a marked lane's read behind it stays inside this object)
    double tile_extra[kTileExtraCells];   // cells kTileRingCells .. of the image tile
    DevBlob B;
    TraceArgs Ab;
    QueueLds<BLOCK / 64, HistRings> Q;
  };
  static_assert(sizeof(RadialLds) % 8 == 0 && (kRadialMarked + 1) * sizeof(double) <= sizeof(RadialLds) + kTileExtraCells * sizeof(double),
                "entry kRadialMarked of either column lies in the table or in the tile's cells");
  __shared__ LdsLayout lds;
  TablesLds& S = lds.S;
  QueueLds<BLOCK / 64, HistRings>& Q = lds.Q;
  static_assert(!PATHC || (FAST && !ROT && GAS >= 0), "the constant-path form belongs to the unrotated specialisations");
  static_assert(!SCAN || GAS != 0, "a mass scan needs the gas stage");
  static_assert(!SCAN || kScanMaxMasses * 2 * kScanLanes <= (BLOCK / 64) * kQueue, "the scan accumulators live in the image tile's 128 doubles per wave");
  __shared__ uint32_t scan_zero[kScanMaxMasses];   // SCAN: rays whose weight vanishes for one mass only (conversion probability exactly 0)
  static_assert(!BANDS || SCAN, "the bands belong to the mass scan");
  __shared__ uint32_t scan_band_n[BANDS ? kScanLanes : 1];   // BANDS: rays of out.m_passed per band cell
  static_assert((BLOCK / 64) * kQueue == kTileRingCells && kImageTileMax * kImageTileMax <= kTileRingCells + kTileExtraCells &&
                    kImageTileExtraMax * kImageTileExtraMax <= kTileExtraCells && BLOCK / 64 == kTileRingCells / kQueue,
                "the LDS image tile (host: kImageTileMax): 128 doubles per wave of this workgroup's rings + the cells behind the tables");
  static_assert((offsetof(LdsLayout, Q) % 512) == 0, "the rings are addressed with ds_*2st64 offsets (units of 512 bytes for 64-bit columns)");
  // cell t < kTileRingCells of the tile space: 128 doubles per wave, in the space of ring 0 (stage A0 off) or of ring 1's path
  // column (PATHC); the scan's accumulators live there
  auto tile_cell_lo = [&](uint32_t t) -> double* {
    return PATHC ? &Q.w[t >> 7].path[t & 127u] : reinterpret_cast<double*>(&Q.w[t >> 7].ray[0]) + (t & 127u);
  };
  // cell t of the LDS image tile: the ring space first, then the cells behind the tables
  auto tile_cell = [&](uint32_t t) -> double* {
    return t < (uint32_t)kTileRingCells ? tile_cell_lo(t) : &lds.tile_extra[t - (uint32_t)kTileRingCells];
  };
  // Only the ~20 scalars phase A needs for every ray travel in the kernel arguments (SGPRs); everything
  // else is read from an LDS copy of the parameter blob (broadcast ds_read).  All of them together do not
  // fit the 102 SGPRs of a wave and would be spilled through VGPR lanes (v_readlane = VALU slots).
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
    // zeroed rings: a slot that was never written reads as ray 0 / shell 0 / radius 0 / u = 0 instead of arbitrary bits
    uint64_t* q = reinterpret_cast<uint64_t*>(&Q);
    for (int i = threadIdx.x; i < (int)(sizeof(Q) / 8); i += BLOCK) q[i] = 0ull;
    for (int i = threadIdx.x; i < kTileExtraCells; i += BLOCK) lds.tile_extra[i] = 0.0;
    if (SCAN && threadIdx.x < kScanMaxMasses) scan_zero[threadIdx.x] = 0u;   // (the barrier of stage_tables orders both before their first use)
    if (BANDS && threadIdx.x < kScanLanes) scan_band_n[threadIdx.x] = 0u;
  }
  // The radial verdict table of the solar-source specialisations (HotA::radial_table: the host could build it for this setup).
  constexpr bool RTAB = FAST;
  if (RTAB && (CFG::kFoldA1 ? CFG::kRadialTable : H.radial_table)) {
    const auto src = as_global(reinterpret_cast<const uint64_t*>(Tb.shell_lut + kRadialTableOffset));
    uint64_t* dst = reinterpret_cast<uint64_t*>(&lds.R);
    for (int i = threadIdx.x; i < kRadialTableCells; i += BLOCK) dst[i] = src[i];
  }
  stage_tables<BLOCK>(S, Pb, Tb, RTAB && (CFG::kFoldA1 ? CFG::kRadialTable : H.radial_table));
  const LdsTables L{S.sincos, S.rcdf_hi, Tb.flux_radius_cdf, S.rguide, S.shells, S.lut, &lds.R, &Tb};

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave-uniform: scalar addressing of the rings
  const uint64_t waves_total = (uint64_t)gridDim.x * (BLOCK / 64);
  const uint64_t wave_global = (uint64_t)blockIdx.x * (BLOCK / 64) + wave;
  // wave-uniform; the host builds no zones for the X-ray test source.  (SCAN without PATHC: ring 0 holds the scan accumulators.)
  const bool early_reject = (SCAN && !PATHC) ? false : (CFG::kFoldAcc ? CFG::kZones : H.n_zones > 0);
  // chunks of 256 ids aligned in global-id space; `rel` = id - id_base (fits 32 bits: n_rays < 2^31)
  const uint64_t first_chunk = A.ray_id_offset >> 8;
  uint64_t id_base = first_chunk << 8;
  // a value of its own: computed in place it stays a part of the eight-register tuple the launch arguments were loaded into, and a
  // phase-A pass that wants it back from the spill lanes reloads all eight
  asm volatile("" : "+s"(id_base));
  const uint32_t rel_begin = (uint32_t)(A.ray_id_offset & 255u);
  const uint32_t rel_end = rel_begin + (uint32_t)A.n_rays;          // one past the last ray (n_rays < 2^31)
  const uint32_t n_chunks = (rel_end + 255u) >> 8;

  // wave-uniform counters (ballot + popcount) and per-lane sums
  uint32_t n_reached = 0, n_shell = 0, n_nickel = 0, n_till = 0, n_passed = 0;
  uint32_t n_outside = 0;    // per lane: passed rays outside the image
  using Sum = std::conditional_t<FIXED, long long, double>;   // per-lane sums: quanta (FIXED) or f64
  Sum sum_w = 0, sum_w2 = 0, sum_x = 0, sum_y = 0, sum_r = 0;
  long long sum_wo = 0;      // FIXED: weights of the passed rays outside the image (the finalize kernel's conservation check)
#ifdef SART_STAGE_TIMING   // diagnostic build (make STAGE_TIMING=1): shader-clock cycles per stage, summed over waves, in scalars 12..15
  uint64_t cyc_a0 = 0, cyc_a1 = 0, cyc_b = 0, cyc_bs[6] = {0, 0, 0, 0, 0, 0};
#endif
  uint32_t h0 = 0, t0 = 0;   // ring 0 (A0 -> A1) positions, monotone; slot = pos % kQueue
  uint32_t h1 = 0, t1 = 0;   // ring 1 (A1 -> B)

  // LDS accesses of one wave execute in order; the fences only keep the compiler from reordering them
  auto ring_sync = [] {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  auto prefix_from = [](uint64_t mask, uint32_t base) {   // base + number of set mask bits below this lane (v_mbcnt adds to its operand)
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, base));
  };

  // The seven sine / cosine coefficients of phase A (sincos_coef()'s values) in vector registers for the whole kernel, where the
  // instantiation has them to spare - vacuum stage, specialised: 107 / 108 of 128 VGPRs without them, the gas and generic ones
  // stand at 114 - 123: 14 s_mov_b32 less per phase-A pass, and the scalar registers they occupied across the three
  // evaluations no longer push kernel-argument pointers into spill lanes (variant 5: 23 -> 12 scalar spills).  The empty asm
  // keeps the compiler from folding the values back into literals.
  constexpr bool HOLD_SINCOS = SART_A_SINCOS_VGPR && FAST && GAS == 0 && !SCAN;
  SinCosCoef Ksc = {-0.5992645293207921, 2.5501640398773455, -5.16771278004997, 3.141592653589793, -1.3352627688545895, 4.0587121264167685,
                    -4.934802200544679};
  if constexpr (HOLD_SINCOS) asm volatile("" : "+v"(Ksc.s3), "+v"(Ksc.s2), "+v"(Ksc.s1), "+v"(Ksc.s0), "+v"(Ksc.d3), "+v"(Ksc.d2), "+v"(Ksc.d1));
  // stage A1 for the ray with id id_base + rel (valid lanes only count); u3_hi = its word of the shared stream
  auto run_phase_a = [&](uint32_t rel, bool valid, uint32_t u3_hi) {
    SART_STAGE_MARK("A1");
    __builtin_amdgcn_s_setprio(SART_PRIO_A1);
    RayState st;
    bool sampled = false, reached = false;
    double radial;
    HotA Hl;
    reload_hot(Hl);
    constexpr bool ZEXT = FAST && !ROT && GAS >= 0;
    LaneMasks M;
    double r3sq = 0.0;
    (void)phase_a<FAST, ROT ? 1 : 0, ZEXT, PATHC, true, RTAB, CFG>(Hl, Pb, L, A.seed_lo, A.seed_hi, id_base + (uint64_t)rel, u3_hi, st, sampled, reached, radial,
                                                              M, HOLD_SINCOS ? &Ksc : nullptr, ROT ? nullptr : &r3sq);
    const uint64_t valid_m = ballot64(valid);
    n_reached += (uint32_t)__popcll(valid_m & M.reached);
    const uint64_t selected = valid_m & M.ok;
    n_shell += (uint32_t)__popcll(selected);
    // A shell above DevParams::mirror_miss_radius (+infinity when the host proved nothing: the block is skipped), the ray at
    // z = l_mirror more than kMirrorMissEps (in mm^2) inside the paraboloid's radius r3 there, and a slope below the bound: the first
    // mirror's quadratic is negative over the whole mirror, pick_root accepts no root, the nickel test is true (sart_api.hip:
    // mirror_miss_bounds_of), and all phase B makes of the ray is +1 in N_HIT_NICKEL.  Counted here, not handed on.  Direct
    // compares, masks combined in scalar registers.
    // (Not compiled into the rotated-telescope instantiations and skipped on a scalar compare for the cone telescope: the host proves
    // nothing for either.)
    uint64_t sure = 0ull;
    // (RTAB: phase A hands both radial compares on as lane masks - from the verdict table where the setup has one, in which case
    // n1_r3sq of the selected shell is read here, where it is needed.)
    const uint64_t cand = (ROT || (CFG::kFoldA1 ? CFG::kIsLlnl : Hl.telescope_kind == SART_TK_LLNL)) ? 0ull
                                                                     : (selected & (RTAB ? M.cand : ballot64(radial > (double)Pb.mirror_miss_radius)));
    if (cand) {   // wave-uniform
      if (RTAB && (CFG::kFoldA1 ? CFG::kRadialTable : Hl.radial_table)) r3sq = L.shells[st.shell].n1_r3sq;
      const double zl = Pb.l_mirror, xe = fma(zl, st.tsx, st.X0), ye = fma(zl, st.tsy, st.Y0);
      sure = cand & ballot64(fma(xe, xe, fma(ye, ye, kMirrorMissEps)) < r3sq) &
             ballot64(fma(st.tsx, st.tsx, st.tsy * st.tsy) < (double)Pb.mirror_miss_slope_sq);
      n_nickel += (uint32_t)__popcll(sure);
    }
    // Innermost shell, far enough below its first mirror (DevParams::shell0_miss_radius; -1 when the host could not prove it): phase
    // B would find no root inside the mirror and stop at the no-hit test without touching a counter.  Such a ray is counted
    // above and ends here.  Below the bound the selected shell is shell 0 (the bound lies below R1[0]): ONE compare against a
    // broadcast read of the parameter block in LDS, whose lane mask is combined with `selected` in scalar registers (the
    // ballot of a direct compare is the compare itself; a ballot of `a && b` costs a select and a second compare).
#ifdef SART_DEBUG_KNOBS
    const uint64_t mask = (A.flags & 0x10000000u) ? 0ull : (selected & (RTAB ? M.keep : ~ballot64(radial < Pb.shell0_miss_radius)) & ~sure);   // experiment: nothing reaches phase B
#else
    const uint64_t mask = selected & (RTAB ? M.keep : ~ballot64(radial < Pb.shell0_miss_radius)) & ~sure;
#endif
    const bool alive = __builtin_amdgcn_inverse_ballot_w64(mask);
    const uint32_t cnt = (uint32_t)__popcll(mask);
    if (alive) {
      asm volatile("; hot: ring 1 write");
      const uint32_t slot = prefix_from(mask, t1) % kQueue;
      Q.w[wave].X0[slot] = st.X0; Q.w[wave].Y0[slot] = st.Y0;
      Q.w[wave].tsx[slot] = st.tsx; Q.w[wave].tsy[slot] = st.tsy;
      if (!PATHC) Q.w[wave].path[slot] = st.path_cb;
      Q.w[wave].cell[slot] = make_uint2((uint32_t)(st.r_idx | (st.shell << 16)), st.u5_hi);
    }
    t1 += cnt;
    __builtin_amdgcn_s_setprio(0);
  };

  auto run_phase_b = [&](uint32_t n_valid) {
    SART_STAGE_MARK("B");
#ifdef SART_STAGE_TIMING
    const uint64_t tb_entry = __builtin_readcyclecounter();
#endif
    __builtin_amdgcn_s_setprio(SART_PRIO_B);
    RayState st;
    const bool valid = (uint32_t)lane < n_valid;
    const uint32_t slot = (h1 + (uint32_t)lane) % kQueue;
    RayOut out;
    {
      // slots beyond n_valid hold the state of earlier rays (or the zeros the rings start with): lanes compute on them
      // predicated off; every index they lead to is one a real ray produced
      st.X0 = Q.w[wave].X0[slot]; st.Y0 = Q.w[wave].Y0[slot];
      st.tsx = Q.w[wave].tsx[slot]; st.tsy = Q.w[wave].tsy[slot];
      st.path_cb = PATHC ? H.length_b : Q.w[wave].path[slot];   // PATHC: z extent of the path = lengthB for every ray
      const uint2 cell = Q.w[wave].cell[slot];
      st.u5 = u52(cell.y, 0u);   // the same bits phase A would have carried as a double
      st.u5_hi = cell.y;
      if (!ROT) {
        st.zcb = -(H.dz3 - H.dz1);
      } else {
        // z of pointExitCB in the rotated frame, recomputed from the ray instead of carried through ring 1 (zcb_rotated)
        st.zcb = zcb_rotated(Pb.rx_s, -Pb.rx_c * Pb.ry_s, Pb.rx_c * Pb.ry_c, Pb.half_length_telescope, st.X0 + Pb.entrance_x,
                             st.Y0 + Pb.entrance_y, st.tsx, st.tsy, H.dz3 - H.dz1);
      }
      const int packed = (int)cell.x;
      st.r_idx = packed & 0xFFFF;
      st.shell = packed >> 16;
      const DevBlob& Bo = lds_opaque(B);
      HotB HB;
      reload_kernarg(HB, offsetof(HistKernArgs, HB));
      // (one round trip beside the ring reads above, not a second one in the middle of the pass)
      asm volatile("" :: "s"(HB.cdf_hi32), "s"(HB.energy_guide), "s"(HB.energy_records), "s"(HB.records_on), "s"(HB.energy_tab), "s"(HB.refl), "s"(HB.refl_n_angles), "s"(HB.cdf_stride));
      phase_b<false, FAST, GAS, FAST && !ROT && GAS >= 0, SCAN, false, false, CFG>(Bo.P, L, HB, lds_opaque(Ab), st, (!FAST && H.test_active) ? Pb.n_energies : -1, valid, out, nullptr);
      if constexpr (SCAN) {
        SART_STAGE_MARK("SCAN");
        // (the per-mass loop stays at phase B's priority: 23.8 against 24.2 ms per 32-mass scan with it below phase A)
        // out.m_passed: rays on the chip whose mass-independent weight factor out.weight is not zero.  Per mass: weight =
        // out.weight x conversion probability (the single-mass kernels multiply in the same order), accumulated per lane.
        n_passed += (uint32_t)__popcll(out.m_passed);
        struct { int32_t n_masses, pad; } hdr;   // (pad: ScanArgs::n_bands)
        reload_kernarg(hdr, offsetof(HistKernArgs, SC));
        const uint32_t fl = (uint32_t)__builtin_amdgcn_readfirstlane((int)Ab.flags);
        const bool use_prob = !(fl & SART_CF_IGNORE_CONV_PROB) & ((GAS >= 0) ? (GAS == 1) : (__builtin_amdgcn_readfirstlane(Bo.P.stage_gas) != 0));
        const double term1 = Bo.P.gas_term1;
        const GasCos cos_lead = GasCos::make();      // (two vector register pairs for the whole loop)
        uint32_t cell = 0u;   // BANDS: the ray's cell among the kScanLanes of a mass and quantity is its energy band
        if constexpr (BANDS) {
          // the band table: the spare words of the first two entries (sart_device.h: ScanMass::aux); wave-uniform
          struct { int32_t e0; uint32_t mul; } b0;
          struct { uint32_t window, unused; } b1;
          reload_kernarg(b0, offsetof(HistKernArgs, SC) + offsetof(ScanArgs, m) + offsetof(ScanMass, aux));
          reload_kernarg(b1, offsetof(HistKernArgs, SC) + offsetof(ScanArgs, m) + sizeof(ScanMass) + offsetof(ScanMass, aux));
          const uint32_t d = (uint32_t)(out.e_idx - b0.e0);   // (an index below e0 wraps to beyond the window)
          // (the mask only bounds what a lane outside out.m_passed computes from an index nobody drew: it adds nothing anywhere)
          cell = (d < b1.window ? __umulhi(2u * d + 1u, b0.mul) : (uint32_t)hdr.pad) & (kScanLanes - 1u);
          if (__builtin_amdgcn_inverse_ballot_w64(out.m_passed))
            __hip_atomic_fetch_add(&scan_band_n[cell], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        for (int k = 0; k < hdr.n_masses; ++k) {   // wave-uniform
          asm volatile("; hot: per-mass loop of the fused scan");
          ScanMass M;   // (staging the table in LDS and reading it one entry ahead instead of this scalar load: -1.5 %, not kept)
          reload_kernarg(M, offsetof(HistKernArgs, SC) + offsetof(ScanArgs, m) + (size_t)k * sizeof(ScanMass));
          double w = out.weight;
          if (use_prob) w *= gas_conversion_prob(M.dm2_abs, out.gas, term1, L.sincos, cos_lead);
          const uint64_t nz = out.m_passed & ballot64(w != 0.0);
          if (nz != out.m_passed) {
            asm volatile("; rare: a conversion probability of exactly zero");
            if (lane == 0) atomicAdd(&scan_zero[k], (uint32_t)__popcll(out.m_passed & ~nz));
          }
          if (__builtin_amdgcn_inverse_ballot_w64(nz)) {
            // cell [k][0][lane % 32]; [k][1][.] is kScanLanes further on (lanes l and l + 32 add to the same cell: the LDS unit
            // takes a wave's 64-bit atomics in groups of lanes, the two never meet in one group)
            // (BANDS: the lanes of one band share a cell, which the LDS unit serialises)
            const uint32_t t = (uint32_t)k * (2u * kScanLanes) + (BANDS ? cell : ((uint32_t)lane & (kScanLanes - 1u)));
            if constexpr (FIXED) {
              __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(tile_cell_lo(t)), (unsigned long long)to_fixed(w, M.fx_scale_w),
                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(tile_cell_lo(t + kScanLanes)), (unsigned long long)to_fixed(w * w, M.fx_scale_w2),
                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            } else {
              __hip_atomic_fetch_add(tile_cell_lo(t), w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              __hip_atomic_fetch_add(tile_cell_lo(t + kScanLanes), w * w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
          }
        }
      }
    }
    h1 += n_valid;
    if constexpr (SCAN) {
      n_nickel += (uint32_t)__popcll(out.m_nickel);
      __builtin_amdgcn_s_setprio(0);
      return;
    }
    __builtin_amdgcn_s_setprio(SART_PRIO_ACC);
#ifdef SART_STAGE_TIMING
    for (int k = 0; k < 5; ++k) cyc_bs[k] += out.tb[k + 1] - out.tb[k];
    cyc_bs[5] += out.tb[0] - tb_entry;   // the ring reads and the argument reload in front of phase B; what follows stamp 5 is the B span minus the six
#endif
    n_nickel += (uint32_t)__popcll(out.m_nickel);
    n_till += (uint32_t)__popcll(out.m_till);
    n_passed += (uint32_t)__popcll(out.m_passed);
    if (out.passed) {
      SART_STAGE_MARK("ACC");
      // the launch's image parameters, re-read from the kernel arguments (scalar registers, short-lived)
      TraceArgs Al;
      reload_kernarg(Al, offsetof(HistKernArgs, A));
      // ONE scalar-memory round trip for everything the accumulation reads: left alone the compiler sinks the loads of the tile and
      // replica parameters into the nested regions that use them - three dependent waits of a scalar load each per pass
      asm volatile("" :: "s"(Al.replicas), "s"(Al.replica_mask), "s"(Al.replica_stride), "s"(Al.image_nx), "s"(Al.image_ny),
                   "s"(Al.image_x_min), "s"(Al.image_y_min), "s"(Al.image_inv_step_x), "s"(Al.image_inv_step_y), "s"(Al.spectra),
                   "s"(Al.tile_x0), "s"(Al.tile_y0), "s"(Al.tile_n), "s"(Al.tile_base));
      long long w_fx = 0;   // FIXED: this ray's weight in quanta (what the image, the sums and the spectra add)
      if constexpr (FIXED) {
        w_fx = to_fixed(out.weight, Al.fx_scale_w);
        sum_w += w_fx;
        sum_w2 += to_fixed(out.weight * out.weight, Al.fx_scale_w2);
        sum_x += to_fixed(out.px, kFixedPositionScale);
        sum_y += to_fixed(out.py, kFixedPositionScale);
        sum_r += to_fixed(out.rdet, kFixedPositionScale);
      } else {
        sum_w += out.weight;
        sum_w2 = fma(out.weight, out.weight, sum_w2);
        sum_x += out.px;
        sum_y += out.py;
        sum_r += out.rdet;
      }
      // prepareHeatmap (:838-842): img[floor(y / step_y), floor(x / step_x)] += w
      // floor(t) in [0, n) <=> 0 <= t < n, and the conversion to int truncates = floor for t >= 0
      const double fx = (out.px - Al.image_x_min) * Al.image_inv_step_x;
      const double fy = (out.py - Al.image_y_min) * Al.image_inv_step_y;
      const int nx = Al.image_nx, ny = Al.image_ny;
      // (lane masks of the four compares combined on the scalar unit; ballots in here see the passed lanes only)
      const uint64_t inside_m = ballot64(fx >= 0.0) & ballot64(fx < (double)nx) & ballot64(fy >= 0.0) & ballot64(fy < (double)ny);
      const bool inside = __builtin_amdgcn_inverse_ballot_w64(inside_m);
      // per lane: this region runs under the lane mask of the passed rays, and a wave-uniform count added in here lands in a
      // vector register whose lane 0 - the one the epilogue reads - only sees the passes in which its own ray passed
      n_outside += inside ? 0u : 1u;
      if constexpr (FIXED) {
        if (out.m_passed & ~inside_m) {   // wave-uniform: no ray of a wave is outside for images that cover the chip
          asm volatile("; rare: passed rays outside the image");
          sum_wo += inside ? 0ll : w_fx;
        }
      }
      // this wave's replica of the image; the pixel's byte offset is 32-bit (image < 2^29 pixels, checked on the host)
#ifdef SART_DEBUG_KNOBS
      const uint32_t rep_key = (Al.flags & 0x08000000u) ? blockIdx.x : (uint32_t)wave_global;   // experiment: replica per XCD
      double* const img = Al.replicas + (size_t)(rep_key & Al.replica_mask) * (size_t)Al.replica_stride;
#else
      double* const img = Al.replicas + (size_t)((uint32_t)wave_global & Al.replica_mask) * (size_t)Al.replica_stride;
#endif
#ifdef SART_DEBUG_KNOBS
      if (inside && !(Al.flags & 0x40000000u))   // SART_DEBUG_NO_IMAGE_ATOMICS (experiment builds only)
#else
      if (inside)
#endif
      {
        const uint32_t ix = (uint32_t)(int)fx, iy = (uint32_t)(int)fy;
        // the workgroup's LDS tile around the focal spot first ("LDS then global atomics"): scattered f64 atomics execute at
        // the memory side, one 64-byte request per lane, ~2e10 / s for the whole chip
        const uint32_t tn = (uint32_t)Al.tile_n;
        const uint32_t tx = ix - (uint32_t)Al.tile_x0, ty = iy - (uint32_t)Al.tile_y0;   // unsigned: below the origin wraps to huge
        if ((tx < tn) & (ty < tn)) {
          const uint32_t t = ty * tn + tx + (uint32_t)Al.tile_base;          // < kTileRingCells + kTileExtraCells (host: tile size per base)
          if constexpr (FIXED)
            __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(tile_cell(t)), (unsigned long long)w_fx, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_WORKGROUP);                                             // ds_add_u64
          else
            __hip_atomic_fetch_add(tile_cell(t), out.weight, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // ds_add_f64
        } else {
          const uint32_t pix = iy * (uint32_t)nx + ix;
          typedef __attribute__((address_space(1))) char* gbytes;
          if constexpr (FIXED) atomic_add_slot_i64((double*)((gbytes)img + pix * 8u), w_fx);
          else unsafeAtomicAdd((double*)((gbytes)img + pix * 8u), out.weight);
        }
      }
      if (CFG::kFoldAcc ? CFG::kSpectra : Al.spectra) {   // wave-uniform: radial and per-energy histograms behind the scalars
        double* rad = acc + (size_t)nx * (size_t)ny + SART_ACC_COUNT;
        double* en = rad + 2 * (size_t)Al.n_radial_bins;
        const size_t ne1 = (size_t)Pb.n_energies + 1;
        const int rb = min((int)(out.rdet * Al.radial_inv_bin), Al.n_radial_bins - 1);
        if constexpr (FIXED) {
          atomic_add_slot_i64(&rad[rb], 1);
          atomic_add_slot_i64(&rad[(size_t)Al.n_radial_bins + rb], w_fx);
          atomic_add_slot_i64(&en[out.e_idx], 1);
          atomic_add_slot_i64(&en[ne1 + out.e_idx], w_fx);
          atomic_add_slot_i64(&en[2 * ne1 + out.e_idx], to_fixed(out.reflect, kFixedReflectScale));
        } else {
          unsafeAtomicAdd(&rad[rb], 1.0);
          unsafeAtomicAdd(&rad[(size_t)Al.n_radial_bins + rb], out.weight);
          unsafeAtomicAdd(&en[out.e_idx], 1.0);
          unsafeAtomicAdd(&en[ne1 + out.e_idx], out.weight);
          unsafeAtomicAdd(&en[2 * ne1 + out.e_idx], out.reflect);
        }
      }
    }
    __builtin_amdgcn_s_setprio(0);
  };

  // Zone bounds of stage A0.  The specialised variants have vector registers to spare (<= 120 of 128) and keep the eight bounds
  // there, one copy per lane, for the whole kernel: the compares read them as they are.  (Re-read from the kernel arguments
  // per pass - what the generic variants do - every stage-A0 pass waits for a scalar-memory round trip with nothing to put
  // in front of it; held in scalar registers they would be spilled through VGPR lanes.)
  constexpr bool kZonesInVgprs = FAST;
  uint32_t zone_lo_v[kMaxZones], zone_hi_v[kMaxZones];
#pragma unroll
  for (int z = 0; z < kMaxZones; ++z) {
    zone_lo_v[z] = H.zone_lo[z];
    zone_hi_v[z] = H.zone_hi[z];
    if (kZonesInVgprs) asm volatile("" : "+v"(zone_lo_v[z]), "+v"(zone_hi_v[z]));   // opaque: stays in a vector register
  }
  uint32_t zone_reached_v = H.zone_reached;   // (one v_readfirstlane per pass: a scalar register held across the loop would push another value out)
  if (kZonesInVgprs) asm volatile("" : "+v"(zone_reached_v));
  uint32_t chunk = (uint32_t)wave_global;                            // relative to first_chunk (wave-uniform)
  const uint32_t lane4 = 4u * (uint32_t)lane;
  uint32_t pass = 0;                                                 // 0..3: which of its four ids a lane handles now
  U4 stream = U4{0u, 0u, 0u, 0u};                                    // this lane's block of the shared word stream
#ifdef SART_STAGE_TIMING
  const uint64_t cyc_start = __builtin_readcyclecounter();
  const uint64_t real_start = __builtin_amdgcn_s_memrealtime();   // constant 100 MHz: shader clock = d(memtime) / d(memrealtime) x 100 MHz
#define SART_STAMP(var) const uint64_t var = __builtin_readcyclecounter()
#define SART_SPAN(acc, t_begin) acc += __builtin_readcyclecounter() - (t_begin)
#else
#define SART_STAMP(var)
#define SART_SPAN(acc, t_begin)
#endif
  for (;;) {
    const bool have_new = chunk < n_chunks;   // wave-uniform
    SART_STAGE_MARK("LOOP");
    if (have_new) {
      SART_STAGE_MARK("A0");
      SART_STAMP(ts_a0);
      if (pass == 0u) {
        asm volatile("; hot x0.25: one block of the shared word stream per four passes");
        stream = stream_block(((first_chunk + (uint64_t)chunk) << 6) + (uint64_t)lane, A.seed_lo, A.seed_hi);
      }
      // high word of u3 (:418) of this pass' ray: the block's next word, with the block moved down by one word behind it.  (Picked by
      // `pass` - word_of() - the wave-uniform index becomes a chain of seven scalar branches in every pass.)
      const uint32_t w = stream.x;
      stream.x = stream.y; stream.y = stream.z; stream.z = stream.w;
      const uint32_t rel = ((chunk << 8) + pass) + lane4;
      if (early_reject) {
        // ---- stage A0: the word against the zones (lane masks and scalar arithmetic only) ----
        ZoneTable Z;
        if constexpr (!kZonesInVgprs) reload_zones(Z);
        const uint32_t zone_reached = kZonesInVgprs ? (uint32_t)__builtin_amdgcn_readfirstlane((int)zone_reached_v) : Z.zone_reached;
        // One word of the stream against the zones: the lane masks of its survivors (`mask`) and of its dead rays that count as
        // having reached the telescope (`reached`).  `zr` and `ck` are zone_reached and chunk as the caller holds them: the second
        // word of a wide pass hands in copies the compiler cannot tell from new values, so that its two wave-uniform tests are a
        // compare and a branch of their own like the first word's, not lane masks of booleans carried from there (+13 scalar
        // instructions per iteration when they were, wide pass or not).
        struct WordMasks { uint64_t mask, reached; };
        auto a0_masks = [&](uint32_t ww, uint32_t rr, uint32_t zr, uint32_t ck) -> WordMasks {
          // lane masks of direct compares (v_cmp writes them) and scalar arithmetic on the masks; the final mask becomes the
          // EXEC mask of the ring write as it is (inverse ballot), with no per-lane 0 / 1 in between
          uint64_t dead_m = 0, in_first = 0;
#pragma unroll
          for (int z = 0; z < kMaxZones; ++z) {   // unused zones are empty: lo > hi
            const uint64_t in = kZonesInVgprs ? (ballot64(ww >= zone_lo_v[z]) & ballot64(ww <= zone_hi_v[z]))
                                              : (ballot64(ww >= Z.lo[z]) & ballot64(ww <= Z.hi[z]));
            dead_m |= in;
            if (z == 0) in_first = in;
          }
          // Only the first zone can be one whose rays do not count as having reached the telescope (sart_api.hip: build_zones puts
          // the zone of kind (a) in front, every zone behind it is of kind (b)): ONE wave-uniform select, not one per zone.
          const uint64_t reached_m = dead_m & ~((zr & 1u) ? 0ull : in_first);
          // all four ids of every lane lie inside the launch for every chunk but the first and the last (wave-uniform test)
          // (only chunk 0 can begin below rel_begin and only chunk n_chunks - 1 can end above rel_end: ONE unsigned compare finds both)
          uint64_t valid_m = ~0ull;
          if (ck - 1u >= n_chunks - 2u) valid_m = ballot64(rr >= rel_begin) & ballot64(rr < rel_end);
#ifdef SART_DEBUG_KNOBS
          const uint64_t mask = (A.flags & 0x20000000u) ? 0ull : (valid_m & ~dead_m);   // experiment: nothing reaches stage A1
#else
          const uint64_t mask = valid_m & ~dead_m;
#endif
          return WordMasks{mask, valid_m & reached_m};
        };
        auto ring0_push = [&](uint64_t mask, uint32_t ww, uint32_t rr) {   // the survivors' ids and words behind what ring 0 holds, in lane order
          if (__builtin_amdgcn_inverse_ballot_w64(mask)) {
            asm volatile("; hot: ring 0 write");
            const uint32_t slot = prefix_from(mask, t0) % kQueue;
            Q.w[wave].ray[slot] = rr;
            Q.w[wave].u3hi[slot] = ww;
          }
          t0 += (uint32_t)__popcll(mask);
        };
        // Invariant: ring 0 holds n0 = t0 - h0 <= 64 entries here (the glue below takes 64 out whenever it holds 64 or more, and an
        // iteration puts in at most kQueue - n0), so the first word's <= 64 survivors always fit its kQueue = 128 slots.
        const WordMasks wa = a0_masks(w, rel, zone_reached, chunk);
        n_reached += (uint32_t)__popcll(wa.reached);
        ring0_push(wa.mask, w, rel);
        // The wide pass (HotA::zone_reached bits kA0WideBit + 0 and + 2, set by the host where the zones retire enough rays:
        // sart_api.hip, a0_wide_rule; bit kA0WideBit + pass: ONE shift and test says "switched on and an even pass"): the lane's
        // next word - id rel + 1 - goes through the same compares in the same iteration, BEHIND the first word's ring write, if
        // ring 0 has room for all of its survivors; one trip through the glue below then serves 128 ids.  If it has not,
        // nothing of the word is counted or written and the next pass - an odd one, never wide - takes it as its one word: every
        // id enters ring 0 once, in the order of the one-word loop, and stage A1 pops the same 64 entries [64 j, 64 j + 64)
        // either way.  The loop ends: every iteration with input takes at least one word.
        if ((zone_reached >> (pass + (uint32_t)kA0WideBit)) & 1u) {   // wave-uniform
          uint32_t zr = zone_reached, ck = chunk;
          asm volatile("" : "+s"(zr), "+s"(ck));
          const uint32_t wb = stream.x;
          const WordMasks mb = a0_masks(wb, rel + 1u, zr, ck);
          if ((t0 - h0) + (uint32_t)__popcll(mb.mask) <= (uint32_t)kQueue) {
            n_reached += (uint32_t)__popcll(mb.reached);
            ring0_push(mb.mask, wb, rel + 1u);
            stream.x = stream.y; stream.y = stream.z; stream.z = stream.w;
            pass += 1u;   // (even before: no carry out of the two bits)
          }
          // (else - rare: the second word does not fit ring 0 and the next, one-word pass takes it again.  No block with a marker
          // of its own: an `else` that holds one turns the test above into a lane mask of a boolean and a second branch on it, three
          // scalar instructions in every wide pass; the fall-back itself has nothing to execute.)
        }
      } else {
        run_phase_a(rel, (rel >= rel_begin) & (rel < rel_end), w);   // no early-rejection stage for this configuration
      }
      pass = (pass + 1u) & 3u;
      if (pass == 0u) chunk += (uint32_t)waves_total;
      ring_sync();
      SART_SPAN(cyc_a0, ts_a0);
    }
    SART_STAGE_MARK("LOOP");
    if (early_reject) {
      // ---- stage A1 on a full wave of A0 survivors (or on the remainder once the input is exhausted) ----
      // (the drain's conditions in blocks of their own, which a wave with input left jumps over: written as one expression they are
      // ten scalar instructions in every iteration)
      const uint32_t n0 = t0 - h0;
      bool a1_due = n0 >= 64u;
      if (chunk >= n_chunks) {   // (compared again, on the scalar unit: `have_new` carried here is a lane mask rebuilt with two vector instructions)
        asm volatile("; the drain");   // (keeps the block a block: no select form)
        a1_due = n0 > 0u;
      }
      if (a1_due) {
        const uint32_t m = min(n0, 64u);
        const bool v = (uint32_t)lane < m;
        const uint32_t slot = (h0 + (uint32_t)lane) % kQueue;
        // slots beyond m hold ids of earlier rays (the rings are zeroed at the start): lanes there trace a ray nobody counts
        const uint32_t rel = Q.w[wave].ray[slot];
        const uint32_t w = Q.w[wave].u3hi[slot];
        h0 += m;
        SART_STAMP(ts_a1);
        run_phase_a(rel, v, w);
        ring_sync();
        SART_SPAN(cyc_a1, ts_a1);
      }
    }
    // ---- stage B on a full wave of A1 survivors (or on the remainder at the very end) ----
    SART_STAGE_MARK("LOOP");
    const uint32_t n1 = t1 - h1;
    bool b_due = n1 >= 64u, draining = false;
    if (chunk >= n_chunks) {
      asm volatile("; the drain");   // (keeps the block a block: no select form)
      draining = t0 == h0;
      b_due |= draining & (n1 > 0u);
    }
    if (b_due) {
      SART_STAMP(ts_b);
      run_phase_b(min(n1, 64u));
      ring_sync();
      SART_SPAN(cyc_b, ts_b);
    }
    if (draining) {
      asm volatile("; the drain");   // (keeps the block a block: no select form)
      if (t1 == h1) break;
    }
  }

  SART_STAGE_MARK("EPILOGUE");
  if constexpr (SCAN) {
    // per-mass sums of this workgroup: a wave adds up the accumulator cells of a mass (a wave-wide sum over a cell per lane: the
    // order is fixed) -> one plain store per mass and quantity, folded by fold_scan_kernel.  One wave-wide read covers [k][0][.]
    // and [k][1][.]: lanes 0 .. 31 hold the sum-of-w cells, lanes 32 .. 63 the sum-of-w^2 cells.
    __syncthreads();   // every wave of the workgroup has left the loop
    static_assert(2 * kScanLanes == 64, "one cell per lane");
    for (int k = wave; k < SCarg.n_masses; k += BLOCK / 64) {
      using Sum = std::conditional_t<FIXED, long long, double>;
      Sum* const dst = reinterpret_cast<Sum*>(SCarg.partials) + ((size_t)blockIdx.x * kScanMaxMasses + (size_t)k) * kScanPartialSlots;
      const double cell = *tile_cell_lo((uint32_t)k * 64u + (uint32_t)lane);
      Sum v;
      if constexpr (FIXED) v = __double_as_longlong(cell); else v = cell;
      if constexpr (BANDS)   // the cells themselves: [workgroup][mass][sum of w: 32 cells | sum of w^2: 32 cells]
        (reinterpret_cast<Sum*>(SCarg.partials) + (size_t)gridDim.x * (kScanMaxMasses * kScanPartialSlots))[(size_t)blockIdx.x * kScanBandSlots + (size_t)k * 64u + (size_t)lane] = v;
#pragma unroll
      for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);   // within each half of the wave
      if (lane == 0) { dst[0] = v; dst[2] = (Sum)scan_zero[k]; dst[3] = 0; }
      if (lane == 32) dst[1] = v;
    }
    if constexpr (BANDS) {
      using Sum = std::conditional_t<FIXED, long long, double>;
      if (threadIdx.x < kScanLanes)   // the per-band counts: the row behind the masses
        (reinterpret_cast<Sum*>(SCarg.partials) + (size_t)gridDim.x * (kScanMaxMasses * kScanPartialSlots))[(size_t)blockIdx.x * kScanBandSlots + kScanMaxMasses * 64u + threadIdx.x] =
            (Sum)scan_band_n[threadIdx.x];
    }
  }
  // flush of the LDS image tile: one global atomic per non-empty tile pixel and workgroup
  if (!SCAN && A.tile_n > 0) {
    __syncthreads();   // every wave of the workgroup has left the loop (uniform condition: kernel argument)
    const uint32_t tn = (uint32_t)A.tile_n, n_tile = tn * tn;
    double* const img = A.replicas + (size_t)((uint32_t)wave_global & A.replica_mask) * (size_t)A.replica_stride;
    for (uint32_t t = threadIdx.x; t < n_tile; t += BLOCK) {
      const double v = *tile_cell(t + (uint32_t)A.tile_base);
      if (__double_as_longlong(v) != 0ll) {   // FIXED: the cell holds an integer; f64: +0.0 is all zero bits, too
        const uint32_t ty = t / tn, tx = t - ty * tn;
        double* const px = &img[(size_t)((uint32_t)A.tile_y0 + ty) * (size_t)A.image_nx + ((uint32_t)A.tile_x0 + tx)];
        if constexpr (FIXED) atomic_add_slot_i64(px, __double_as_longlong(v));
        else unsafeAtomicAdd(px, v);
      }
    }
  }

  // scalars: wave reduction -> LDS -> one plain store per workgroup and quantity (folded by fold_scalars_kernel)
  // (FIXED: the slots hold int64 - sums in quanta, counters as integers - and are added as integers all the way)
  // (the staging area is the head of wave 0's rings - X0, Y0, tsx: dead once every wave has left the loop, and apart from the
  // image tile / the scan accumulators, which live in the path or the ring-0 columns)
  static_assert(sizeof(Sum) * (BLOCK / 64) * SART_ACC_COUNT <= 3 * kQueue * sizeof(double) && offsetof(HistRings, Y0) == kQueue * sizeof(double) &&
                    offsetof(HistRings, tsx) == 2 * kQueue * sizeof(double), "the scalar staging area fits the first three ring columns of wave 0");
  __syncthreads();
  Sum (*const red)[SART_ACC_COUNT] = reinterpret_cast<Sum (*)[SART_ACC_COUNT]>(&Q.w[0].X0[0]);
  Sum sw, sw2, sxx, syy, srr;
  if constexpr (FIXED) {
    sw = wave_sum_i64(sum_w); sw2 = wave_sum_i64(sum_w2); sxx = wave_sum_i64(sum_x); syy = wave_sum_i64(sum_y); srr = wave_sum_i64(sum_r);
  } else {
    sw = wave_sum(sum_w); sw2 = wave_sum(sum_w2); sxx = wave_sum(sum_x); syy = wave_sum(sum_y); srr = wave_sum(sum_r);
  }
  const long long swo = FIXED ? wave_sum_i64(sum_wo) : 0ll;
  const long long n_out = wave_sum_i64((long long)n_outside);   // (a per-lane count, see the accumulation)
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
#ifdef SART_STAGE_TIMING
    r[12] = (Sum)cyc_a0; r[13] = (Sum)cyc_a1; r[14] = (Sum)cyc_b;
    r[15] = (Sum)(__builtin_readcyclecounter() - cyc_start);
    r[SART_ACC_N_HIT_NICKEL] = (Sum)(__builtin_amdgcn_s_memrealtime() - real_start);
    // sub-stages of B, packed two per slot (each < 2^40, slot = hi * 2^40 + lo would lose bits in f64): use the sums of x/y/r slots
    r[SART_ACC_SUM_X] = (Sum)cyc_bs[0]; r[SART_ACC_SUM_Y] = (Sum)cyc_bs[1]; r[SART_ACC_SUM_R] = (Sum)cyc_bs[2];
    r[SART_ACC_SUM_WEIGHTS_SQ] = (Sum)cyc_bs[3]; r[SART_ACC_N_OUTSIDE_IMAGE] = (Sum)cyc_bs[4]; r[SART_ACC_SUM_WEIGHTS] = (Sum)cyc_bs[5];
#endif
  }
  __syncthreads();
  if (threadIdx.x < SART_ACC_COUNT) {
    Sum t = 0;
    for (int w = 0; w < BLOCK / 64; ++w) t += red[w][threadIdx.x];
    reinterpret_cast<Sum*>(A.partials)[(size_t)blockIdx.x * SART_ACC_COUNT + threadIdx.x] = t;
  }
