// The x2-phase streaming kernel of keep_conv_x3s.hip (its comment: "x2 phases, streaming"), included there twice: XU_KERNEL = the kernel's name,
// XU_X1 = false (KEEP_MMA_X3, conv3x3_up2_x3s_kernel) or true (KEEP_MMA_X1 with KEEP_CONV_X1_UP2, conv3x3_up2_x1s_kernel).  One text, two PLAIN
// kernels -- not a kernel template: as a template instantiation (or behind an inlined template body) the x3 form compiles to another
// instruction stream than the one profiles/up2_stream_ab.txt measured (other spill slots around the item transitions).
__global__ __launch_bounds__(256, 2) void XU_KERNEL(ConvP p, int tiles_x, int tiles_y, int ncb, int n_items) {
  constexpr bool X1 = XU_X1;
  constexpr int WB = X1 ? 2 : 4;               // bytes per weight of p.wx3
  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[XU_LDS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lhi = lane >> 5, g = tid & 3;
  const int nch = p.Cin >> 4;                  // chunks per item (>= 2: host)
  if ((int)blockIdx.x >= n_items) return;

  auto make_rsrc = [&](const void* ptr, int bytes) __attribute__((always_inline)) {
    const unsigned long long b = (unsigned long long)ptr;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)hi << 32) | lo), 0, bytes, 0x00020000);
  };
  const __amdgpu_buffer_rsrc_t null_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.in, 0, 0, 0x00020000);   // every offset out of range: zeros, no traffic
  const int w_phase = p.Cout * 9 * p.Cin * WB; // bytes of one phase kernel (4 of them < 2^31: host)
  const __amdgpu_buffer_rsrc_t w_rsrc = make_rsrc(p.wx3, 4 * w_phase);

  // With two phases' accumulators (128 registers) the pipeline's own working set leaves nothing for values that only the item transitions
  // and the epilogue use: those are recomputed there from an OPAQUE copy of the thread index, so that they are not kept alive across the MFMA loops
  auto opaque = [](int x) __attribute__((always_inline)) {
    asm volatile("" : "+v"(x));
    return x;
  };
  // ---- per-thread constants: the halo image, its swizzle and the fragment addresses are those of conv3x3_halo_x3s_kernel
  int wr_addr[HALO_IT];
#pragma unroll
  for (int k = 0; k < HALO_IT; ++k) {
    const int hp = (tid >> 2) + k * 64;
    const int hx = hp % XS_HW;
    wr_addr[k] = hp < XS_PIX ? hp * 64 + (((g >> 1) ^ ((hx >> 2) & 3)) << 4) + (g & 1) * 8 : XS_PIX * 64 + lane * 8;
  }
  int rd_aM[3];                                // kw -> pixel (2 wave + py, l31 + kw) of the halo, py = the row parity of item M
#pragma unroll
  for (int kw = 0; kw < 3; ++kw) rd_aM[kw] = ((2 * wave) * XS_HW + l31 + kw) * 64 + ((lhi ^ (((l31 + kw) >> 2) & 3)) << 4);
  const int rd_b = XS_WOFF + l31 * 64 + ((lhi ^ ((l31 >> 2) & 3)) << 4);

  // an item: (image, source tile, row parity, cout block) -- the parity rides as the upper half of 2 ncb virtual cout blocks; HaloItem::z
  // (the split-K slice of the other kernels: always 0 here) carries it
  auto decode = [&](int item) __attribute__((always_inline)) {
    HaloItem it = halo_decode<32, 4>(p, item, n_items, tiles_x, tiles_y, 2 * ncb);
    const int cbv = it.n0 >> 6;
    it.z = cbv >= ncb ? 1 : 0;
    it.n0 = (cbv - it.z * ncb) << 6;
    return it;
  };

  // ---- pipeline state (F / C / M as above)
  HaloItem itF = decode(blockIdx.x), itC = itF, itM = itF;
  itM.z = 0;                                   // rd_aM starts at parity 0: enter_M() moves it by the difference
  int chF = 0, chC = 0, chM = 0, itemF = blockIdx.x;
  bool okF = true, okC = false;
  int h_voff[HALO_IT];
  __amdgpu_buffer_rsrc_t in_rsrc = null_rsrc;
  float amaxF = 0.f;
  int dma_voff = -16;                          // C: this lane's source offset inside a (phase, tap) slab: cout n0 + 16 wave + lane / 4
  int dma_soff = 0;                            // C: py * (two phase kernels + one tap row)
  float in_sC = 1.f, in_invC = 1.f, in_invM = 1.f;
  bool after_epi = false;
  float4 biasM = make_float4(0.f, 0.f, 0.f, 0.f);

  auto setup_F = [&]() __attribute__((always_inline)) {
    const int t_ = opaque(tid);
#pragma unroll
    for (int k = 0; k < HALO_IT; ++k) {
      const int hp = (t_ >> 2) + k * 64;
      h_voff[k] = -16;
      if (hp < XS_PIX) {
        const int hy = hp / XS_HW, hx = hp - hy * XS_HW;
        const int iy = itF.oy0 - 1 + hy, ix = itF.ox0 - 1 + hx;
        if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) h_voff[k] = ((iy * p.W + ix) * p.in_ld + (t_ & 3) * 4) * 4;
      }
    }
    in_rsrc = make_rsrc(p.in + (long)itF.n * p.H * p.W * p.in_ld, p.H * p.W * p.in_ld * 4);
    if (p.in_amax) amaxF = p.in_amax[itF.n];
  };
  auto cross_C = [&]() __attribute__((always_inline)) {
    const int t_ = opaque(tid);
    const int lp = (t_ & 3) ^ ((t_ >> 4) & 3);
    const int co = itF.n0 + (t_ >> 6) * 16 + ((t_ & 63) >> 2);
    dma_voff = co < p.Cout ? co * 9 * p.Cin * WB + lp * 16 : -16;
    dma_soff = __builtin_amdgcn_readfirstlane(itF.z * (2 * w_phase + 3 * p.Cin * WB));
    in_sC = 1.f;
    in_invC = 1.f;
    if (p.in_amax) x3_range_scale(amaxF, in_sC, in_invC);
  };
  auto enter_M = [&]() __attribute__((always_inline)) {      // M <- C at an item's first chunk
    const int dpy = (itC.z - itM.z) * (XS_HW * 64);
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) rd_aM[kw] += dpy;
    itM = itC;
    in_invM = in_invC;
  };
  auto advance_F = [&]() __attribute__((always_inline)) {
    if (++chF < nch) return;
    chF = 0;
    itemF += gridDim.x;
    okF = itemF < n_items;
    if (okF) {
      itF = decode(itemF);
      setup_F();
    }
  };

  float4 hreg[HALO_IT];
  float cv[4] = {0.f, 0.f, 0.f, 0.f}, cw[4] = {0.f, 0.f, 0.f, 0.f};
  f16x2 chi[2] = {f16x2{(_Float16)0.f, (_Float16)0.f}, f16x2{(_Float16)0.f, (_Float16)0.f}};
  f16x2 clo[2] = {f16x2{(_Float16)0.f, (_Float16)0.f}, f16x2{(_Float16)0.f, (_Float16)0.f}};
  f32x16 acc[2][2][2];                         // [px][i][j]

  // conversion of piece k = q / 16, step q % 16 (the raw-input form of the kernel above in the first seven of the piece's 16 gaps)
  auto conv_step = [&](int q, int hb) __attribute__((always_inline)) {
    if constexpr (X1) {                        // piece k = q / 5, steps 0 .. 3 of its five gaps: one rounding, no `lo`
      const int k = q / 5, st = q % 5;
      const float rs = p.in_amax ? in_sC : 1.f;
      if (st == 0) { cv[0] = hreg[k].x * rs; cv[1] = hreg[k].y * rs; }
      if (st == 1) {
        cv[2] = hreg[k].z * rs; cv[3] = hreg[k].w * rs;
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(okF ? in_rsrc : null_rsrc, h_voff[k], chF * 64, KEEP_LD_AUX_XS);
        hreg[k] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
      }
      if (st == 2) {
        chi[0] = __builtin_convertvector(f32x2{cv[0], cv[1]}, f16x2);
        chi[1] = __builtin_convertvector(f32x2{cv[2], cv[3]}, f16x2);
      }
      if (st == 3)
        *reinterpret_cast<uint2*>(lds_raw + wr_addr[k] + hb) = make_uint2(__builtin_bit_cast(unsigned, chi[0]), __builtin_bit_cast(unsigned, chi[1]));
      return;
    }
    const int k = q / 16, st = q % 16;
    const float rs = p.in_amax ? in_sC : 1.f;
    if (st == 0) { cv[0] = hreg[k].x * rs; cv[1] = hreg[k].y * rs; }
    if (st == 1) {
      cv[2] = hreg[k].z * rs; cv[3] = hreg[k].w * rs;
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(okF ? in_rsrc : null_rsrc, h_voff[k], chF * 64, KEEP_LD_AUX_XS);
      hreg[k] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
    }
    if (st == 2) {
      chi[0] = __builtin_convertvector(f32x2{cv[0], cv[1]}, f16x2);
      chi[1] = __builtin_convertvector(f32x2{cv[2], cv[3]}, f16x2);
    }
    if (st == 3) { cw[0] = __builtin_fmaf((float)chi[0].x, -1.0f, cv[0]); cw[1] = __builtin_fmaf((float)chi[0].y, -1.0f, cv[1]); }
    if (st == 4) { cw[2] = __builtin_fmaf((float)chi[1].x, -1.0f, cv[2]); cw[3] = __builtin_fmaf((float)chi[1].y, -1.0f, cv[3]); }
    if (st == 5) {
      clo[0] = __builtin_convertvector(f32x2{cw[0], cw[1]}, f16x2);
      clo[1] = __builtin_convertvector(f32x2{cw[2], cw[3]}, f16x2);
      *reinterpret_cast<uint2*>(lds_raw + wr_addr[k] + hb) = make_uint2(__builtin_bit_cast(unsigned, chi[0]), __builtin_bit_cast(unsigned, chi[1]));
    }
    if (st == 6)
      *reinterpret_cast<uint2*>(lds_raw + (wr_addr[k] ^ 32) + hb) = make_uint2(__builtin_bit_cast(unsigned, clo[0]), __builtin_bit_cast(unsigned, clo[1]));
  };
  // weights of chunk C, virtual taps 3 gq .. (3 gq + 2 | 7): one 1 KB piece (16 cout rows) per wave and virtual tap
  auto dma_group = [&](int gq) __attribute__((always_inline)) {
    const int wq = __builtin_amdgcn_readfirstlane(wave);
#pragma unroll
    for (int v = 3 * gq; v < (gq == 2 ? 8 : 3 * gq + 3); ++v) {
      const int px = v & 1, s = v >> 1;
      const int tap_rel = (s >> 1) * 3 + px + (s & 1);          // kh * 3 + kw less the parity's 3 py
      __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rsrc, (__attribute__((address_space(3))) void*)(lds_raw + XS_WOFF + (4 * v + wq) * 1024), 16, dma_voff,
                                               X1 ? dma_soff + px * w_phase + tap_rel * p.Cin * 2 + (chC >> 1) * 64
                                                  : dma_soff + px * w_phase + (tap_rel * p.Cin + chC * 16) * 4, 0, 0);
    }
  };
  // fragments of virtual tap t: 0 a_lo0, 1 a_lo1, 2 b_hi0, 3 b_hi1, 4 a_hi0, 5 a_hi1, 6 b_lo0, 7 b_lo1
  auto frag_of = [&](int t, int f, int hb) __attribute__((always_inline)) -> f16x8 {
    const int px = t & 1, s = t >> 1, kh = s >> 1, kw = px + (s & 1);
    if (f == 0 || f == 1 || f == 4 || f == 5) {
      const int i = f & 1;
      const int a = (f < 4 ? (rd_aM[kw] ^ 32) : rd_aM[kw]) + hb + ((i + kh) * XS_HW) * 64;
      return *reinterpret_cast<const f16x8*>(lds_raw + a);
    }
    const int j = f & 1;
    const int o = (f >= 4 ? (rd_b ^ 32) : rd_b) + (t * 64 + j * 32) * 64;
    return *reinterpret_cast<const f16x8*>(lds_raw + o);
  };
  auto mma_step = [&](int hbM, int hbC) __attribute__((always_inline)) {
    if constexpr (X1) {
      const int rd_bM = rd_b ^ ((chM & 1) << 5);        // the chunk's half of the two-chunk weight rows
      auto frag1 = [&](int t, int f) __attribute__((always_inline)) -> f16x8 {      // 0 a0, 1 a1, 2 b0, 3 b1 of virtual tap t
        const int px = t & 1, s = t >> 1, kh = s >> 1, kw = px + (s & 1);
        if (f < 2) return *reinterpret_cast<const f16x8*>(lds_raw + rd_aM[kw] + hbM + ((f + kh) * XS_HW) * 64);
        return *reinterpret_cast<const f16x8*>(lds_raw + rd_bM + (t * 64 + (f - 2) * 32) * 64);
      };
      f16x8 fr[2][4];
#pragma unroll
      for (int f = 0; f < 4; ++f) fr[0][f] = frag1(0, f);
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int px = t & 1;
        const bool new_a = !(t == 1 || t == 5);  // virtual tap t + 1 reads other halo pixels than t
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const int i = m >> 1, j = m & 1;
          acc[px][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fr[t & 1][i], fr[t & 1][2 + j], acc[px][i][j], 0, 0, 0);
          if (t < 7) fr[(t + 1) & 1][m] = (m < 2 && !new_a) ? fr[t & 1][m] : frag1(t + 1, m);
          if (t * 4 + m < 5 * HALO_IT) conv_step(t * 4 + m, hbC);
          __builtin_amdgcn_sched_barrier(0);
        }
        if (t == 2) {          // the weight ring and its counted waits: see the x3 loop below (requests of gaps 1, 6 and 11 are younger than group 2)
          if (after_epi) {
            asm volatile("s_waitcnt vmcnt(35)" ::: "memory");
          } else {
            asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
          }
          asm volatile("s_barrier" ::: "memory");
          if (okC && !(chC & 1)) dma_group(0);
          __builtin_amdgcn_sched_barrier(0);
        }
        if (t == 5) {
          asm volatile("s_barrier" ::: "memory");
          if (okC && !(chC & 1)) dma_group(1);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      return;
    }
    f16x8 fr[8];
#pragma unroll
    for (int f = 0; f < 8; ++f) fr[f] = frag_of(0, f, hbM);
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int px = t & 1;
      const bool new_a = !(t == 1 || t == 5);  // virtual tap t + 1 reads other halo pixels than t
#pragma unroll
      for (int m = 0; m < 12; ++m) {
        const int term = m >> 2, i = (m >> 1) & 1, j = m & 1;
        const int ia = term == 0 ? i : 4 + i;
        const int ib = term == 1 ? 6 + j : 2 + j;
        acc[px][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fr[ia], fr[ib], acc[px][i][j], 0, 0, 0);
        if (t < 7) {            // re-read behind the last use: a_lo0 m=1, a_lo1 3, b_lo0 6, b_lo1 7, a_hi0 9, b_hi0 10, a_hi1 / b_hi1 11
          if (m == 1 && new_a) fr[0] = frag_of(t + 1, 0, hbM);
          if (m == 3 && new_a) fr[1] = frag_of(t + 1, 1, hbM);
          if (m == 6) fr[6] = frag_of(t + 1, 6, hbM);
          if (m == 7) fr[7] = frag_of(t + 1, 7, hbM);
          if (m == 9 && new_a) fr[4] = frag_of(t + 1, 4, hbM);
          if (m == 10) fr[2] = frag_of(t + 1, 2, hbM);
          if (m == 11) {
            if (new_a) fr[5] = frag_of(t + 1, 5, hbM);
            fr[3] = frag_of(t + 1, 3, hbM);
          }
        }
        conv_step(t * 12 + m, hbC);
        __builtin_amdgcn_sched_barrier(0);
      }
      // The weight ring (see the kernel above).  Group 2 of this chunk went out behind the previous step's last barrier and is published by
      // the first ring barrier: the vector-memory instructions younger than it are at least this step's requests of gaps 1, 17 and 33 --
      // behind an epilogue also its 2 x 16 output stores.
      if (t == 2) {
        if (after_epi) {
          asm volatile("s_waitcnt vmcnt(35)" ::: "memory");
        } else {
          asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        }
        asm volatile("s_barrier" ::: "memory");
        if (okC) dma_group(0);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (t == 5) {
        asm volatile("s_barrier" ::: "memory");
        if (okC) dma_group(1);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };

  // ---- epilogue of item itM: phase by phase, 16 pixel rows at a time through the halo buffer the item's last chunk just released; per phase
  // the arithmetic and the order of the sums are conv3x3_halo_x3_kernel's (pixel groups 0..15 per lane, the two lane-swap sums, waves in order)
  auto epilogue_t = [&](int hb, auto res_c) __attribute__((always_inline)) {
    constexpr bool HAS_RES = decltype(res_c)::value;
    const int t_ = opaque(tid);
    const int lane = t_ & 63, wave = t_ >> 6, l31 = lane & 31, lhi = lane >> 5;      // (shadow the kernel's: see `opaque`)
    float* et = reinterpret_cast<float*>(lds_raw + hb) + wave * 16 * XS_EP;
    const float asc = p.acc_scale * in_invM;
    const int c4 = (lane & 15) * 4, prow = lane >> 4;
    const int co = itM.n0 + c4;
    const bool cok = co < p.Cout;
    const int hw_o = p.Ho * p.Wo;
    const int py = itM.z;
    const __amdgpu_buffer_rsrc_t out_rsrc = make_rsrc(p.out + (long)itM.n * hw_o * p.out_ld, hw_o * p.out_ld * 4);
    __amdgpu_buffer_rsrc_t res_rsrc = out_rsrc;
    if (HAS_RES) res_rsrc = make_rsrc(p.res + (long)itM.n * hw_o * p.res_ld, hw_o * p.res_ld * 4);
    const float4 bias4 = biasM;
    float amx = 0.f;
    auto dpix_of = [&](int q16) __attribute__((always_inline)) { return 2 * ((q16 >> 3) * p.Wo + (q16 & 7) * 4); };      // source pixel group -> output pixels, stride 2
#pragma unroll
    for (int px = 0; px < 2; ++px) {
      // source pixel (y, x) of phase (py, px) -> output pixel (2 y + py, 2 x + px)
      const int pix_b = (2 * (itM.oy0 + 2 * wave) + py) * p.Wo + 2 * (itM.ox0 + prow) + px;
      const int v_out = cok ? (pix_b * p.out_ld + co) * 4 : -16;
      const int v_res = HAS_RES && cok ? (pix_b * p.res_ld + co) * 4 : -16;
      float s4[4] = {0.f, 0.f, 0.f, 0.f}, ss4[4] = {0.f, 0.f, 0.f, 0.f};
      // the residual rows of an accumulator tile (8 pixel groups) before the tile's first store (in place a thread reads exactly what it
      // later writes; tiles and phases are disjoint): with two phases' accumulators live there are no registers for a whole phase's 16
      u32x4 rpre[HAS_RES ? 8 : 1];
#pragma unroll
      for (int rd = 0; rd < 4; ++rd) {
        if (HAS_RES && !(rd & 1)) {
#pragma unroll
          for (int q8 = 0; q8 < 8; ++q8) rpre[q8] = __builtin_amdgcn_raw_buffer_load_b128(res_rsrc, v_res, dpix_of(rd * 4 + q8) * p.res_ld * 4, KEEP_LD_AUX_RES);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r8 = 0; r8 < 8; ++r8) {
            const int r = (rd & 1) * 8 + r8;
            et[((r & 3) + 8 * ((r >> 2) & 1) + 4 * lhi) * XS_EP + j * 32 + l31] = acc[px][rd >> 1][j][r];
          }
        __builtin_amdgcn_s_waitcnt(0xc07f);      // lgkmcnt(0): wave-local hand-off
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float4 v = *reinterpret_cast<const float4*>(et + (u * 4 + prow) * XS_EP + c4);
          float e[4] = {__builtin_fmaf(v.x, asc, bias4.x), __builtin_fmaf(v.y, asc, bias4.y), __builtin_fmaf(v.z, asc, bias4.z),
                        __builtin_fmaf(v.w, asc, bias4.w)};
          if (HAS_RES) {
            const u32x4 r4 = rpre[HAS_RES ? (rd & 1) * 4 + u : 0];
            e[0] += __uint_as_float(r4.x); e[1] += __uint_as_float(r4.y);
            e[2] += __uint_as_float(r4.z); e[3] += __uint_as_float(r4.w);
          }
          u32x4 o;
          o.x = __float_as_uint(e[0]); o.y = __float_as_uint(e[1]); o.z = __float_as_uint(e[2]); o.w = __float_as_uint(e[3]);
          __builtin_amdgcn_raw_buffer_store_b128(o, out_rsrc, v_out, dpix_of(rd * 4 + u) * p.out_ld * 4, KEEP_ST_AUX_XS);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            s4[q] += e[q];
            ss4[q] = __builtin_fmaf(e[q], e[q], ss4[q]);
            amx = fmaxf(amx, fabsf(e[q]));
          }
          // one pixel group's values at a time: left alone, the sums are sunk into the `p.stats` branch below and the values of all 16 groups
          // of the phase stay in registers until then (64 registers: scratch)
          asm volatile("" : "+v"(s4[0]), "+v"(s4[1]), "+v"(s4[2]), "+v"(s4[3]), "+v"(ss4[0]), "+v"(ss4[1]), "+v"(ss4[2]), "+v"(ss4[3]), "+v"(amx));
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      if (p.stats) {            // the wave's sums of this phase: behind the parked rows, one slab per phase (the next phase parks over the rows)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          s4[q] = xs_xor32_sum(xs_xor16_sum(s4[q]));
          ss4[q] = xs_xor32_sum(xs_xor16_sum(ss4[q]));
        }
        if (lane < 16) {
          float* sw = reinterpret_cast<float*>(lds_raw + hb + XU_STAT + px * 2048) + wave * 128;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            sw[(c4 + q) * 2 + 0] = s4[q];
            sw[(c4 + q) * 2 + 1] = ss4[q];
          }
        }
      }
    }
    if (p.stats) {              // four partials per source tile, one per phase: wave px adds the four waves' sums of phase px in wave order
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      if (wave < 2) {
        const float* e0 = reinterpret_cast<const float*>(lds_raw + hb + XU_STAT + wave * 2048);
        float a = 0.f, b2 = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          a += e0[w * 128 + lane * 2 + 0];
          b2 += e0[w * 128 + lane * 2 + 1];
        }
        if (itM.n0 + lane < p.Cout) {
          const int part = (itM.ty * tiles_x + itM.tx) * 4 + py * 2 + wave;
          float* dst = p.stats + (((long)itM.n * p.stats_P + part) * p.Cout + itM.n0 + lane) * 2;
          dst[0] = a;
          dst[1] = b2;
        }
      }
    }
    return amx;
  };
  auto zero_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[x][i][j][r] = 0.f;
  };

  // ---- prologue: chunk 0 of the block's first item converted in the open, chunk 1 requested
  setup_F();
#pragma unroll
  for (int k = 0; k < HALO_IT; ++k) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(in_rsrc, h_voff[k], 0, KEEP_LD_AUX_XS);
    hreg[k] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
  }
  itC = itF;
  chC = 0;
  okC = true;
  cross_C();
  advance_F();                                 // F: chunk 1 of the same item (nch >= 2)
  dma_group(0);
  dma_group(1);
  dma_group(2);
#pragma unroll
  for (int k = 0; k < HALO_IT; ++k) {
#pragma unroll
    for (int st = 0; st < (X1 ? 5 : 16); ++st) conv_step(k * (X1 ? 5 : 16) + st, 0);
  }
  enter_M();
  chM = 0;
  chC = 1;                                     // C: chunk 1 (same item)
  advance_F();                                 // F: chunk 2, or the next item's chunk 0
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();
  zero_acc();

  int amax_n = -1;
  float amax_run = 0.f;
  auto step = [&](auto hb_c) __attribute__((always_inline)) -> bool {
    constexpr int HB = decltype(hb_c)::value;
    const bool last = chM == nch - 1;
    if (last) {
      const int co = itM.n0 + (opaque(tid) & 15) * 4;
      biasM = make_float4(0.f, 0.f, 0.f, 0.f);
      if (p.bias && co < p.Cout) biasM = *reinterpret_cast<const float4*>(p.bias + co);
    }
    mma_step(HB, XS_HBUF - HB);
    // this wave's weight pieces of groups 0 and 1 and its converted rows are in LDS; younger than the last of those pieces is the
    // raw-piece request of gap 81 (X1: 26) alone
    asm volatile("s_waitcnt vmcnt(1) lgkmcnt(0)" ::: "memory");
    asm volatile("s_barrier" ::: "memory");              // every wave is done with halo buffer HB and virtual taps 6-7; the other buffer and the next groups 0-1 are complete
    if (okC && (!X1 || !(chC & 1))) dma_group(2);
    if (last) {
      const float amx = p.res ? epilogue_t(HB, std::true_type{}) : epilogue_t(HB, std::false_type{});
      if (p.out_amax) {
        if (itM.n != amax_n) {
          amax_n = itM.n;
          amax_run = 0.f;
        }
        if (__builtin_amdgcn_ballot_w64(amx > amax_run) != 0ull) {
          unsigned b = __float_as_uint(amx);
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) b = max(b, (unsigned)__shfl_xor((int)b, o));
          unsigned* dst = p.out_amax + itM.n;
          unsigned seen = b;
          if (lane == 0) {
            seen = *reinterpret_cast<volatile unsigned*>(dst);
            if (b > seen) atomicMax(dst, b);
          }
          seen = max(b, (unsigned)__builtin_amdgcn_readfirstlane((int)seen));
          amax_run = fmaxf(amax_run, __uint_as_float(seen));
        }
      }
      zero_acc();
    }
    after_epi = last;
    if (!okC) return true;
    if (chC == 0) enter_M();
    chM = chC;
    okC = okF;
    if (okF) {
      if (chF == 0) {
        itC = itF;
        cross_C();
      }
      chC = chF;
      advance_F();
    }
    if (last) {                                // the parked rows / statistics of the epilogue live in buffer HB: the next step converts into it
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      asm volatile("s_barrier" ::: "memory");
    }
    return false;
  };
  while (true) {
    if (step(std::integral_constant<int, 0>{})) break;
    if (step(std::integral_constant<int, XS_HBUF>{})) break;
  }
}
