// The body of trace_angular_scan_kernel and of ascan_images_kernel (sart_kernels.hip, which describes it and includes this file once
// inside each of the two: one text, so that the image scan's rows stay the flux-only scan's bit for bit and both kernels compile to
// the code they had as two copies - a shared __device__ function, inlined, does not).  In scope: the template parameters BLOCK, FAST,
// GAS, FIXED, the constant IMAGES, and the kernel's parameters H, blob, A, img_partials, HBarg, ANarg.
  struct LdsLayout {   // the layout of trace_histogram_kernel (tables first: ds_ offsets)
    TablesLds S;
    double cells[kRingExtraCells];
    DevBlob B;
    TraceArgs Ab;
    QueueLds<BLOCK / 64> Q;
  };
  __shared__ LdsLayout lds;
  static_assert((offsetof(LdsLayout, Q) % 512) == 0, "the rings are addressed with ds_*2st64 offsets");
  static_assert(kAScanCells == (BLOCK / 64) * kQueue, "the per-angle cells are the u5 column of the workgroup's rings");
  TablesLds& S = lds.S;
  QueueLds<BLOCK / 64>& Q = lds.Q;
  // per angle: N_PASSED, N_HIT_NICKEL, N_PASSED_TILL_WINDOW, N_SHELL_SELECTED of this workgroup; [4 kAScanMaxAngles]: N_REACHED_TELESCOPE
  uint32_t* const cnt = reinterpret_cast<uint32_t*>(&lds.cells[kAScanCounters]);
  [[maybe_unused]] uint32_t* const cnt_out = reinterpret_cast<uint32_t*>(&lds.cells[kAImgNOutside]);   // IMAGES: N_OUTSIDE_IMAGE per angle
  // cell t of the per-angle sums: slot t % 128 of wave t / 128's u5 column
  auto acc_cell = [&](uint32_t t) -> double* { return &Q.w[t >> 7].u5[t & 127u]; };
  DevBlob& B = lds.B;
  TraceArgs& Ab = lds.Ab;
  (void)img_partials; (void)HBarg;
  {
    const uint64_t* src = reinterpret_cast<const uint64_t*>(blob);
    uint64_t* dst = reinterpret_cast<uint64_t*>(&B);
    for (int i = threadIdx.x; i < (int)(sizeof(DevBlob) / 8); i += BLOCK) dst[i] = src[i];
    if (threadIdx.x == 0) Ab = A;
    uint64_t* q = reinterpret_cast<uint64_t*>(&Q);
    for (int i = threadIdx.x; i < (int)(sizeof(Q) / 8); i += BLOCK) q[i] = 0ull;   // (the rings, and with them the cells)
    if (threadIdx.x < 4 * kAScanMaxAngles + 4) cnt[threadIdx.x] = 0u;
    if constexpr (IMAGES)
      if (threadIdx.x < kAImgCellsEnd - kAImgPos) lds.cells[kAImgPos + threadIdx.x] = 0.0;   // position / outside sums, outside counters
    if (threadIdx.x < 3 * kAScanMaxAngles) {
      // third column of every angle's rotation, from the kernel arguments (a per-thread read of the argument segment)
      typedef const __attribute__((address_space(4))) double* kernarg_f64;
      const kernarg_f64 a0 = (kernarg_f64)((const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr() +
                                           offsetof(AScanKernArgs, AN) + offsetof(AScanArgs, a) + offsetof(AScanAngle, mx));
      const int k = threadIdx.x / 3, j = threadIdx.x - 3 * k;
      lds.cells[kAScanMTable + threadIdx.x] = a0[k * (int)(sizeof(AScanAngle) / 8) + j];
    }
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
  const bool early_reject = H.n_zones > 0;   // wave-uniform; no zones for the X-ray test source
  const uint64_t first_chunk = A.ray_id_offset >> 8;
  uint64_t id_base = first_chunk << 8;
  asm volatile("" : "+s"(id_base));
  const uint32_t rel_begin = (uint32_t)(A.ray_id_offset & 255u);
  const uint32_t rel_end = rel_begin + (uint32_t)A.n_rays;
  const uint32_t n_chunks = (rel_end + 255u) >> 8;
  const int n_angles = ANarg.n_angles;

  uint32_t n_reached = 0;
  uint32_t h0 = 0, t0 = 0, h1 = 0, t1 = 0;
  auto ring_sync = [] {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  auto prefix_of = [](uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
  };

  // the stash: the wave of rays whose angles are being worked through (registers)
  double st_x1 = 0.0, st_y1 = 0.0, st_x3 = 0.0, st_y3 = 0.0, st_path = 0.0;
  int st_eidx = 0;        // energy index of the ray (row n_energies: the X-ray test source's fixed energy)
  uint64_t stash_m = 0;   // its lanes that hold a ray of this launch that reached the telescope
  int ka = n_angles;      // next angle of the stash; n_angles: no stash

  // stage A1a: sample -> bore -> pipes for the ray with id id_base + rel
  auto run_bore = [&](uint32_t rel, bool valid, uint32_t u3_hi) {
    SART_STAGE_MARK("A1a");
    __builtin_amdgcn_s_setprio(SART_PRIO_A1);
    RayState st;
    bool sampled = false, reached = false;
    HotA Hl;
    reload_hot(Hl);
    BoreRay br;
    LaneMasks M;
    phase_a_bore<FAST, false, false, true>(Hl, Pb, L, uniforms_of(A.seed_lo, A.seed_hi, id_base + (uint64_t)rel, u3_hi), st, sampled, reached, br, M);
    stash_m = ballot64(valid) & M.reached;
    n_reached += (uint32_t)__popcll(stash_m);
    st_x1 = br.x1; st_y1 = br.y1; st_x3 = br.x3; st_y3 = br.y3;
    st_path = st.path_cb;
    if (!FAST && Hl.test_active) {   // wave-uniform
      st_eidx = Pb.n_energies;
    } else {
      // getRandomEnergyFromSolarModel (:444-471) once per ray: the three dependent gathers of the draw, here and not in phase B
      // (lanes whose ray is dead draw from a valid row with a valid uniform: the result is not used)
      HotB HB;
      reload_kernarg(HB, offsetof(AScanKernArgs, HB));
      st_eidx = sample_energy_index<true>(HB, st.r_idx, st.u5, st.u5_hi);
    }
    ka = stash_m ? 0 : n_angles;   // (a wave none of whose rays reached the telescope has no angles to walk)
    __builtin_amdgcn_s_setprio(0);
  };

  // stage A1b: the stash through telescope frame, opaque structures and shell selection for angle k (wave-uniform)
  auto run_telescope = [&](int k) {
    SART_STAGE_MARK("A1b");
    __builtin_amdgcn_s_setprio(SART_PRIO_A1);
    HotA Hl;
    reload_hot(Hl);
    struct { TelRot R; double shell0_miss_radius; } ang;   // the head of AScanAngle
    static_assert(offsetof(AScanAngle, rx_c) == 0 && offsetof(AScanAngle, shell0_miss_radius) == sizeof(TelRot), "the head of AScanAngle");
    reload_kernarg(ang, offsetof(AScanKernArgs, AN) + offsetof(AScanArgs, a) + (size_t)k * sizeof(AScanAngle));
    BoreRay br;
    br.x1 = st_x1; br.y1 = st_y1; br.x3 = st_x3; br.y3 = st_y3;
    br.sx = 0.0; br.sy = 0.0;   // (read by the unrotated form only)
    br.ok = __builtin_amdgcn_inverse_ballot_w64(stash_m);
    br.okm = stash_m;
    RayState st;
    st.path_cb = st_path;
    double radial;
    LaneMasks M;
    (void)phase_a_telescope<FAST, 1>(Hl, Pb, ang.R, L, br, st, radial, M);
    const uint64_t selected = M.ok;   // (starts from stash_m: valid, reached)
    if (lane == 0) atomicAdd(&cnt[4 * k + 3], (uint32_t)__popcll(selected));
    // rays that provably miss the first mirror of the innermost shell end here, as in the histogram kernel (this angle's bound)
    const uint64_t mask = selected & ~ballot64(radial < ang.shell0_miss_radius);
    if (__builtin_amdgcn_inverse_ballot_w64(mask)) {
      asm volatile("; hot: ring 1 write");
      const uint32_t slot = (t1 + prefix_of(mask)) % kQueue;
      Q.w[wave].X0[slot] = st.X0; Q.w[wave].Y0[slot] = st.Y0;
      Q.w[wave].tsx[slot] = st.tsx; Q.w[wave].tsy[slot] = st.tsy;
      Q.w[wave].path[slot] = st.path_cb;
      Q.w[wave].idx[slot] = st_eidx | (st.shell << 16) | (k << 24);   // energy index < 2^16 (the guide tables are u16), shell < 64, angle < 32
    }
    t1 += (uint32_t)__popcll(mask);
    __builtin_amdgcn_s_setprio(0);
  };

  // stage B: mirrors -> weight on a wave of ring 1 (rays of several angles), accumulated per angle
  auto run_mirrors = [&](uint32_t n_valid) {
    SART_STAGE_MARK("B");
    __builtin_amdgcn_s_setprio(SART_PRIO_B);
    RayState st;
    const bool valid = (uint32_t)lane < n_valid;
    const uint32_t slot = (h1 + (uint32_t)lane) % kQueue;
    st.X0 = Q.w[wave].X0[slot]; st.Y0 = Q.w[wave].Y0[slot];
    st.tsx = Q.w[wave].tsx[slot]; st.tsy = Q.w[wave].tsy[slot];
    st.path_cb = Q.w[wave].path[slot];
    st.u5 = 0.0;
    st.r_idx = 0;
    const int packed = Q.w[wave].idx[slot];   // (slots beyond n_valid hold earlier rays or zeros: a real ray's indices, angle < n_angles)
    const int e_idx = packed & 0xFFFF;
    st.shell = (packed >> 16) & 0xFF;
    const uint32_t kl = (uint32_t)packed >> 24;
    {
      const double* const m = &lds.cells[kAScanMTable + 3 * kl];
      st.zcb = zcb_rotated(m[0], m[1], m[2], Pb.half_length_telescope, st.X0 + Pb.entrance_x, st.Y0 + Pb.entrance_y, st.tsx, st.tsy,
                           H.dz3 - H.dz1);
    }
    h1 += n_valid;
    const DevBlob& Bo = lds_opaque(B);
    HotB HB;
    reload_kernarg(HB, offsetof(AScanKernArgs, HB));
    asm volatile("" :: "s"(HB.cdf_hi32), "s"(HB.energy_guide), "s"(HB.energy_tab), "s"(HB.refl), "s"(HB.refl_n_angles), "s"(HB.cdf_stride));
    RayOut out;
    phase_b<false, FAST, GAS, false, false, true>(Bo.P, L, HB, lds_opaque(Ab), st, e_idx, valid, out, nullptr);   // (no draw in there)
    SART_STAGE_MARK("ACC");
    __builtin_amdgcn_s_setprio(SART_PRIO_ACC);
    if (__builtin_amdgcn_inverse_ballot_w64(out.m_nickel)) atomicAdd(&cnt[4 * kl + 1], 1u);
    if (__builtin_amdgcn_inverse_ballot_w64(out.m_till)) atomicAdd(&cnt[4 * kl + 2], 1u);
    if (out.passed) {
      atomicAdd(&cnt[4 * kl], 1u);
      // cell [kl][0][lane % 32]; [kl][1][.] is kScanLanes further on (lanes l and l + 32 share a cell, as in the mass scan)
      double* const cell = acc_cell(kl * (2u * kScanLanes) + ((uint32_t)lane & (kScanLanes - 1u)));   // (+ kScanLanes stays inside the wave's column)
      if constexpr (FIXED) {
        double fx_w, fx_w2;
        { const TraceArgs& Al = lds_opaque(Ab); fx_w = Al.fx_scale_w; fx_w2 = Al.fx_scale_w2; }
        __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(cell), (unsigned long long)to_fixed(out.weight, fx_w), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(cell + kScanLanes), (unsigned long long)to_fixed(out.weight * out.weight, fx_w2),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      } else {
        __hip_atomic_fetch_add(cell, out.weight, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(cell + kScanLanes, out.weight * out.weight, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      if constexpr (IMAGES) {
        // what trace_histogram_kernel accumulates for a passed ray, into the block of angle kl (A.replicas: the block of the
        // group's first angle, A.replica_stride: the length of a block): position sums in LDS, the pixel and the spectra with
        // global atomics (no LDS tile: 32 of them do not fit)
        SART_STAGE_MARK("IMG");
        TraceArgs Al;
        reload_kernarg(Al, offsetof(AScanKernArgs, A));
        asm volatile("" :: "s"(Al.replicas), "s"(Al.replica_stride), "s"(Al.image_nx), "s"(Al.image_ny), "s"(Al.image_x_min),
                     "s"(Al.image_y_min), "s"(Al.image_inv_step_x), "s"(Al.image_inv_step_y), "s"(Al.spectra));
        double* const blk = Al.replicas + (size_t)kl * (size_t)Al.replica_stride;
        double* const pos = &lds.cells[kAImgPos + kl * (3u * kAImgLanes) + ((uint32_t)lane & (kAImgLanes - 1u))];
        long long w_fx = 0;
        if constexpr (FIXED) {
          w_fx = to_fixed(out.weight, Al.fx_scale_w);
          __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(pos), (unsigned long long)to_fixed(out.px, kFixedPositionScale),
                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(pos + kAImgLanes), (unsigned long long)to_fixed(out.py, kFixedPositionScale),
                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(pos + 2 * kAImgLanes), (unsigned long long)to_fixed(out.rdet, kFixedPositionScale),
                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
          __hip_atomic_fetch_add(pos, out.px, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          __hip_atomic_fetch_add(pos + kAImgLanes, out.py, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          __hip_atomic_fetch_add(pos + 2 * kAImgLanes, out.rdet, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        // prepareHeatmap (:838-842) with the expressions of trace_histogram_kernel
        const double fx = (out.px - Al.image_x_min) * Al.image_inv_step_x;
        const double fy = (out.py - Al.image_y_min) * Al.image_inv_step_y;
        const int nx = Al.image_nx, ny = Al.image_ny;
        const uint64_t inside_m = ballot64(fx >= 0.0) & ballot64(fx < (double)nx) & ballot64(fy >= 0.0) & ballot64(fy < (double)ny);
        if (__builtin_amdgcn_inverse_ballot_w64(inside_m)) {
          const uint32_t pix = (uint32_t)(int)fy * (uint32_t)nx + (uint32_t)(int)fx;
          if constexpr (FIXED) atomic_add_slot_i64(blk + pix, w_fx);
          else unsafeAtomicAdd(blk + pix, out.weight);
        } else {
          asm volatile("; rare: passed rays outside the image");
          atomicAdd(&cnt_out[kl], 1u);
          if constexpr (FIXED)
            __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(&lds.cells[kAImgOutside + kl]), (unsigned long long)w_fx,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        if (Al.spectra) {   // wave-uniform: radial and per-energy histograms behind the scalars
          double* rad = blk + (size_t)nx * (size_t)ny + SART_ACC_COUNT;
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
    }
    __builtin_amdgcn_s_setprio(0);
  };

  // zone bounds of stage A0 (see trace_histogram_kernel)
  constexpr bool kZonesInVgprs = FAST;
  uint32_t zone_lo_v[kMaxZones], zone_hi_v[kMaxZones];
#pragma unroll
  for (int z = 0; z < kMaxZones; ++z) {
    zone_lo_v[z] = H.zone_lo[z];
    zone_hi_v[z] = H.zone_hi[z];
    if (kZonesInVgprs) asm volatile("" : "+v"(zone_lo_v[z]), "+v"(zone_hi_v[z]));
  }
  uint32_t zone_reached_v = H.zone_reached;
  if (kZonesInVgprs) asm volatile("" : "+v"(zone_reached_v));
  uint32_t chunk = (uint32_t)wave_global;
  const uint32_t lane4 = 4u * (uint32_t)lane;
  uint32_t pass = 0;
  U4 stream = U4{0u, 0u, 0u, 0u};
  for (;;) {
    const bool have_new = chunk < n_chunks;   // wave-uniform
    SART_STAGE_MARK("LOOP");
    if (ka == n_angles) {   // no stash: take rays in until a full wave of them has passed stage A0
      if (have_new) {
        SART_STAGE_MARK("A0");
        if (pass == 0u) stream = stream_block(((first_chunk + (uint64_t)chunk) << 6) + (uint64_t)lane, A.seed_lo, A.seed_hi);
        const uint32_t w = word_of(stream, pass);
        const uint32_t rel = ((chunk << 8) + pass) + lane4;
        pass = (pass + 1u) & 3u;
        if (pass == 0u) chunk += (uint32_t)waves_total;
        if (early_reject) {
          ZoneTable Z;
          if constexpr (!kZonesInVgprs) reload_zones(Z);
          const uint32_t zone_reached = kZonesInVgprs ? (uint32_t)__builtin_amdgcn_readfirstlane((int)zone_reached_v) : Z.zone_reached;
          uint64_t dead_m = 0, reached_m = 0;
#pragma unroll
          for (int z = 0; z < kMaxZones; ++z) {
            const uint64_t in = kZonesInVgprs ? (ballot64(w >= zone_lo_v[z]) & ballot64(w <= zone_hi_v[z]))
                                              : (ballot64(w >= Z.lo[z]) & ballot64(w <= Z.hi[z]));
            dead_m |= in;
            reached_m |= ((zone_reached >> z) & 1u) ? in : 0ull;
          }
          const uint64_t valid_m = ballot64(rel >= rel_begin) & ballot64(rel < rel_end);
          n_reached += (uint32_t)__popcll(valid_m & reached_m);
          const uint64_t mask = valid_m & ~dead_m;
          if (__builtin_amdgcn_inverse_ballot_w64(mask)) {
            asm volatile("; hot: ring 0 write");
            const uint32_t slot = (t0 + prefix_of(mask)) % kQueue;
            Q.w[wave].ray[slot] = rel;
            Q.w[wave].u3hi[slot] = w;
          }
          t0 += (uint32_t)__popcll(mask);
          ring_sync();
        } else {
          run_bore(rel, (rel >= rel_begin) & (rel < rel_end), w);   // no early-rejection stage for this configuration
        }
      }
      SART_STAGE_MARK("LOOP");
      if (early_reject) {
        const uint32_t n0 = t0 - h0;
        if ((n0 >= 64u) | (!have_new & (n0 > 0u))) {
          const uint32_t m = min(n0, 64u);
          const uint32_t slot = (h0 + (uint32_t)lane) % kQueue;
          const uint32_t rel = Q.w[wave].ray[slot];
          const uint32_t w = Q.w[wave].u3hi[slot];
          h0 += m;
          run_bore(rel, (uint32_t)lane < m, w);
        }
      }
    }
    SART_STAGE_MARK("LOOP");
    if (ka < n_angles) {
      run_telescope(ka);
      ++ka;
      ring_sync();
    }
    SART_STAGE_MARK("LOOP");
    const uint32_t n1 = t1 - h1;
    const bool draining = !have_new & (t0 == h0) & (ka == n_angles);
    if ((n1 >= 64u) | (draining & (n1 > 0u))) {
      run_mirrors(min(n1, 64u));
      ring_sync();
    }
    if (draining & (t1 == h1)) break;
  }

  SART_STAGE_MARK("EPILOGUE");
  // per angle: a wave adds up the angle's cells (lanes 0 .. 31: sum of w, lanes 32 .. 63: sum of w^2; fixed order) -> plain stores
  // into this workgroup's partial row, folded by fold_ascan_kernel
  if (lane == 0) atomicAdd(&cnt[4 * kAScanMaxAngles], n_reached);
  __syncthreads();   // every wave has left the loop
  using Sum = std::conditional_t<FIXED, long long, double>;
  for (int k = wave; k < n_angles; k += BLOCK / 64) {
    Sum* const dst = reinterpret_cast<Sum*>(ANarg.partials) + ((size_t)blockIdx.x * kAScanMaxAngles + (size_t)k) * kAScanPartialSlots;
    const double cell = *acc_cell((uint32_t)(k * 64 + lane));
    Sum v;
    if constexpr (FIXED) v = __double_as_longlong(cell); else v = cell;
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);   // within each half of the wave
    if (lane == 0) dst[0] = v;
    if (lane == 32) dst[1] = v;
    if (lane < 4) dst[2 + lane] = (Sum)cnt[4 * k + lane];
    if (lane == 4) dst[6] = (k == 0) ? (Sum)cnt[4 * kAScanMaxAngles] : (Sum)0;
    if (lane == 5) dst[7] = (Sum)0;
    if constexpr (IMAGES) {
      // this workgroup's SART_ACC_COUNT scalars of angle k -> img_partials[k][blockIdx.x][.] (plain stores; fold_scalars_*_kernel
      // per angle, as behind trace_histogram_kernel).  Lanes 0 .. 23: position cells [SUM_X, SUM_Y, SUM_R][kAImgLanes].
      const double pc = (lane < 3 * kAImgLanes) ? lds.cells[kAImgPos + k * (3 * kAImgLanes) + lane] : 0.0;
      Sum p;
      if constexpr (FIXED) p = __double_as_longlong(pc); else p = pc;
#pragma unroll
      for (int off = kAImgLanes / 2; off > 0; off >>= 1) p += __shfl_xor(p, off, 64);   // within each group of kAImgLanes lanes
      const Sum sw = __shfl(v, 0, 64), sw2 = __shfl(v, 32, 64);
      const Sum sx = __shfl(p, 0, 64), sy = __shfl(p, kAImgLanes, 64), sr = __shfl(p, 2 * kAImgLanes, 64);
      Sum s = 0;
      switch (lane) {
        case SART_ACC_SUM_WEIGHTS: s = sw; break;
        case SART_ACC_SUM_WEIGHTS_SQ: s = sw2; break;
        case SART_ACC_SUM_X: s = sx; break;
        case SART_ACC_SUM_Y: s = sy; break;
        case SART_ACC_SUM_R: s = sr; break;
        case SART_ACC_N_PASSED: s = (Sum)cnt[4 * k]; break;
        case SART_ACC_N_HIT_NICKEL: s = (Sum)cnt[4 * k + 1]; break;
        case SART_ACC_N_PASSED_TILL_WINDOW: s = (Sum)cnt[4 * k + 2]; break;
        case SART_ACC_N_SHELL_SELECTED: s = (Sum)cnt[4 * k + 3]; break;
        case SART_ACC_N_REACHED_TELESCOPE: s = (Sum)cnt[4 * kAScanMaxAngles]; break;
        case SART_ACC_N_OUTSIDE_IMAGE: s = (Sum)cnt_out[k]; break;
        case SART_ACC_SUM_WEIGHTS_OUTSIDE: if constexpr (FIXED) s = __double_as_longlong(lds.cells[kAImgOutside + k]); break;
        default: break;   // N_RAYS (the fold adds it), the high limbs (the fold carries into them), the reserved slots
      }
      if (lane < SART_ACC_COUNT) reinterpret_cast<Sum*>(img_partials)[((size_t)k * gridDim.x + blockIdx.x) * SART_ACC_COUNT + lane] = s;
    }
  }
