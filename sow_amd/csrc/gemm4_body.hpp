// gemm4 kernel bodies, included by gemm4.hip once per 16-bit element type (no include guard, on purpose).  Textual rather than a
// template on the element type, so that the bf16 kernels compile from the very same source as before the f16 forms existed
// (a template body inlined into per-type entry points changes the bf16 register allocation).  The includer defines:
//   G4_KERNEL, G4_REDUCE  entry symbols of the main and of the split-K reduction kernel
//   G4_T                  element type (bf16_t / f16_t) of the epilogue's reads of C and bias
//   G4_MFMA               v_mfma_f32_16x16x32_{bf16,f16} on 16-byte register images
//   G4_PACK               fp32 pair -> two RNE-rounded 16-bit elements in one dword
//   G4_ONE                bit pattern of 1.0 (the dbias column of the saved projection)
// Operand loads, LDS-DMA, transposed reads and swizzles move raw 16-bit words and do not depend on the element type.

// SK = the split-K form (its own instantiation: the plain kernel sits at 249-250 VGPRs and must not pay for the K-range
// bookkeeping or the partial-sum epilogue)
template <bool NT, bool HF, bool SK = false> __global__ __launch_bounds__(G4_THREADS, 2) void G4_KERNEL(const Gemm4Params p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wr = w >> 2, wc = w & 3;
  const int r16 = lane & 15, g = lane >> 4;
  const int tiles_n = (p.N + G4_BN - 1) / G4_BN;
  const int splits = SK ? p.splits : 1;
  const int ntiles = (int)gridDim.x / splits;
  const int split = splits > 1 ? (int)blockIdx.x / ntiles : 0;
  const int lid = splits > 1 ? (int)blockIdx.x % ntiles : xcd_remap(blockIdx.x, gridDim.x);
  const int64_t m0 = (int64_t)(lid / tiles_n) * G4_BM;
  const int n0 = (lid % tiles_n) * G4_BN;
  const int K = p.K, N = p.N;
  const int64_t M = p.M;
  const int nfull = K / G4_BK;
  const bool has_ext = HF || p.A2 != nullptr;
  const int NTL_all = nfull + ((K % G4_BK) ? 1 : 0) + (has_ext ? 1 : 0);   // K-tiles of the product
  // this block's K-tiles [kt0, NTL): the whole product, or its split's range (never empty: the launcher sizes kt_per so)
  const int kt0 = splits > 1 ? split * p.kt_per : 0;
  const int NTL = splits > 1 ? (kt0 + p.kt_per < NTL_all ? kt0 + p.kt_per : NTL_all) : NTL_all;
  const int H = 4 * NTL;                                            // half-tiles (global numbering)
  const char* zp = zero_page_for(lane);

  // ------------------------------------------------------------------ DMA geometry (per lane)
  // k-contiguous image [128][64]: instruction ii of this wave covers image rows 16 w + 8 ii .. + 7
  const int c_pc = lane & 7;                                    // physical chunk this lane writes
  int c_lr[2], c_q[2];                                          // image row, logical chunk
#pragma unroll
  for (int ii = 0; ii < 2; ++ii) {
    c_lr[ii] = 16 * w + 8 * ii + (lane >> 3);
    c_q[ii] = c_pc ^ ((c_lr[ii] >> 1) & 7);
  }
  auto a_row = [&](int mh, int lr) -> int64_t {                 // global row of image row lr of A half mh (clamped)
    const int64_t gr = m0 + (lr >> 6) * 128 + mh * 64 + (lr & 63);
    return gr < M ? gr : M - 1;
  };
  auto b_col_nt = [&](int nh, int lr) -> int {                  // global column of image row lr of B half nh (clamped)
    const int gn = n0 + (lr >> 5) * 64 + nh * 32 + (lr & 31);
    return gn < N ? gn : N - 1;
  };
  // k-major image [64 k][128 n]: instruction ii covers k rows 8 w + 4 ii .. + 3
  const int m_kr0 = 8 * w + (lane >> 4);                        // k row of ii = 0 (ii = 1: + 4)
  const int m_f = (((lane >> 4) & 3) | ((w & 1) << 2)) << 1;    // swizzle of that k row (the same for ii = 1)
  const int m_q = (lane & 15) ^ m_f;                            // logical chunk
  auto b_col_nn = [&](int nh) -> int {                          // first global column of this lane's chunk (clamped)
    const int lc = 8 * m_q;
    const int gn = n0 + (lc >> 5) * 64 + nh * 32 + (lc & 31);
    return gn + 8 <= N ? gn : N - 8;
  };

  // per-lane source pointers of the full K-tiles, advanced per tile
  const bf16_t* pA[2][2];
  const bf16_t* pB[2][2];
#pragma unroll
  for (int hh = 0; hh < 2; ++hh)
#pragma unroll
    for (int ii = 0; ii < 2; ++ii) {
      pA[hh][ii] = p.A + a_row(hh, c_lr[ii]) * p.lda + 8 * c_q[ii];
      if constexpr (NT) pB[hh][ii] = p.B + (int64_t)b_col_nt(hh, c_lr[ii]) * p.ldb + 8 * c_q[ii];
      else pB[hh][ii] = p.B + (int64_t)(m_kr0 + 4 * ii) * p.ldb + b_col_nn(hh);
    }
  const int64_t stepB = NT ? (int64_t)G4_BK : (int64_t)G4_BK * p.ldb;
  if (kt0 > 0) {
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
#pragma unroll
      for (int ii = 0; ii < 2; ++ii) pA[hh][ii] += (int64_t)kt0 * G4_BK, pB[hh][ii] += (int64_t)kt0 * stepB;
  }

  // DMA of half-tile KIND of K-tile `tile`
  auto issue = [&](auto kind_c, int tile) {
    constexpr int KIND = decltype(kind_c)::value;
    constexpr bool IS_A = KIND == G4_A0 || KIND == G4_A1;
    constexpr int HH = (KIND == G4_A1 || KIND == G4_B1) ? 1 : 0;
    char* dst = smem + (tile & 1) * G4_BUF + g4_slot_off<KIND>() + (2 * w) * 1024;
    if (tile < nfull) {
#pragma unroll
      for (int ii = 0; ii < 2; ++ii) {
        if constexpr (IS_A) {
          dma16(pA[HH][ii], dst + ii * 1024);
          pA[HH][ii] += G4_BK;
        } else {
          dma16(pB[HH][ii], dst + ii * 1024);
          pB[HH][ii] += stepB;
        }
      }
      return;
    }
    // checked path: the K tail of the main operands, or the extension tile
    const bool ext = has_ext && tile == NTL_all - 1;
    const int k0 = ext ? 0 : nfull * G4_BK;
#pragma unroll
    for (int ii = 0; ii < 2; ++ii) {
      const void* src;
      if constexpr (IS_A) {
        const bf16_t* base = ext ? p.A2 : p.A;
        const int64_t ld = ext ? p.lda2 : p.lda;
        const int klim = ext ? 64 : K;
        const int kk = k0 + 8 * c_q[ii];
        // gemm4h: the extension's A operand is the projected tile in LDS; the DMA slot is filled with zeros only to keep
        // the counted waits uniform
        src = (kk < klim && !(HF && ext)) ? (const void*)(base + a_row(HH, c_lr[ii]) * ld + kk) : (const void*)zp;
      } else if constexpr (NT) {
        const bf16_t* base = ext ? p.B2 : p.B;
        const int64_t ld = ext ? p.ldb2 : p.ldb;
        const int klim = ext ? p.k2e : K;
        const int kk = k0 + 8 * c_q[ii];
        const int64_t eoff = (int64_t)b_col_nt(HH, c_lr[ii]) * ld + kk;
        // gemm4h: B2 = A as stored ([N][r], 2r-byte rows): pieces straddling r carry the next row's head (they meet the
        // exact zeros of H's ranks >= r); the piece that would cross the end of the buffer reads zeros, patched before use
        const bool ok = kk < klim && !(HF && ext && eoff + 8 > (int64_t)N * ld);
        src = ok ? (const void*)(base + eoff) : (const void*)zp;
      } else {
        const bf16_t* base = ext ? p.B2 : p.B;
        const int64_t ld = ext ? p.ldb2 : p.ldb;
        const int krows = ext ? p.k2 : K;
        const int gk = k0 + m_kr0 + 4 * ii;
        src = gk < krows ? (const void*)(base + (int64_t)gk * ld + b_col_nn(HH)) : (const void*)zp;
      }
      dma16(src, dst + ii * 1024);
    }
  };
  using KA0 = std::integral_constant<int, G4_A0>;
  using KB0 = std::integral_constant<int, G4_B0>;
  using KB1 = std::integral_constant<int, G4_B1>;
  using KA1 = std::integral_constant<int, G4_A1>;

  // ------------------------------------------------------------------ gemm4h: projection pass H^T = F' . A^T over all of K
  // A lighter pipeline of its own (HBM-bound: the row panel streams in once, the main loop below re-reads it from L2 /
  // the Infinity Cache): three 40-KiB buffers in the ring, two K-tiles in flight, every wave the same schedule.  Wave
  // (wr, wc) owns rows 128 wr .. + 127 x ranks 16 wc .. + 15 (32 accumulator registers, dead before the main loop starts).
  if constexpr (HF) {
    const int NTA = (K + G4_BK - 1) / G4_BK;
    const int f_row = 8 * w + (lane >> 3);     // NT: rank row of F; NN: k row of the padded [K][64] factor
    const int f_pc = lane & 7;
    const int f_q = NT ? (f_pc ^ ((f_row >> 1) & 7)) : (f_pc ^ ((((lane >> 4) & 1) | ((w & 1) << 1)) << 1));
    auto issue_a = [&](int tl) {
      char* buf = smem + (tl % 3) * G4_PA_BUF;
      const int k0 = tl * G4_BK;
#pragma unroll
      for (int hh = 0; hh < 2; ++hh)
#pragma unroll
        for (int ii = 0; ii < 2; ++ii) {
          const void* src = (k0 + 8 * c_q[ii] < K) ? (const void*)pA[hh][ii] : (const void*)zp;
          dma16(src, buf + hh * G4_HALF + (2 * w + ii) * 1024);
          pA[hh][ii] += G4_BK;
        }
      const void* fs;
      if constexpr (NT) {
        const int kk = k0 + 8 * f_q;
        fs = (f_row < p.r && kk < K) ? (const void*)(p.F + (int64_t)f_row * p.ldf + kk) : (const void*)zp;
      } else {
        // F = A as stored ([K][r], 2r-byte rows, r even): a 16-byte piece may carry the head of the next row -- those are
        // ranks >= r, masked when H is written -- and the ONE piece that would cross the end of the buffer (last row,
        // straddling piece) reads zeros and is patched below
        const int gk = k0 + f_row;
        const int64_t eoff = (int64_t)gk * p.ldf + 8 * f_q;
        const bool ok = gk < K && 8 * f_q < p.r && eoff + 8 <= (int64_t)K * p.ldf;
        fs = ok ? (const void*)(p.F + eoff) : (const void*)zp;
      }
      dma16(fs, buf + 2 * G4_HALF + w * 1024);
    };
    auto patch_f = [&](int tl) {   // after this wave's pieces of tile tl have landed, before the barrier that publishes them
      if constexpr (!NT) {
        const int gk = tl * G4_BK + f_row;
        const int64_t eoff = (int64_t)gk * p.ldf + 8 * f_q;
        if (gk < K && 8 * f_q < p.r && eoff + 8 > (int64_t)K * p.ldf) {
          u32x4 v;
          bf16_t* e = (bf16_t*)&v;
#pragma unroll
          for (int j = 0; j < 8; ++j) e[j] = (8 * f_q + j < p.r) ? p.F[eoff + j] : (bf16_t)0.f;
          *(u32x4*)(smem + (tl % 3) * G4_PA_BUF + 2 * G4_HALF + w * 1024 + lane * 16) = v;
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
      }
    };
    const uint32_t lbase = lds_addr(smem);
    const int fsw_a = (r16 >> 1) & 7;
    const int cha = (fsw_a & 4) | (g ^ (fsw_a & 3));
    const uint32_t ar0 = lbase + (uint32_t)((wr * 64 + r16) * 128 + cha * 16);
    const uint32_t ar1 = lbase + (uint32_t)((wr * 64 + r16) * 128 + (cha ^ 4) * 16);
    uint32_t fr0, fr1;
    if constexpr (NT) {
      fr0 = lbase + (uint32_t)(2 * G4_HALF + (wc * 16 + r16) * 128 + cha * 16);
      fr1 = lbase + (uint32_t)(2 * G4_HALF + (wc * 16 + r16) * 128 + (cha ^ 4) * 16);
    } else {
      const int qq = r16 >> 2, pp = r16 & 3;
      const int ff_sw = (((qq >> 1) & 1) | ((g & 1) << 1)) << 1;
      const int chunk = wc * 2 + (pp >> 1);
      fr0 = lbase + (uint32_t)(2 * G4_HALF + (8 * g + qq) * 128 + ((chunk ^ ff_sw) * 16) + 8 * (pp & 1));
      fr1 = fr0;
    }
    f32x4 hacc[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) hacc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    issue_a(0);
    if (NTA > 1) issue_a(1);
#pragma unroll 1
    for (int tl = 0; tl < NTA; ++tl) {
      wait_groups<5>(NTA - 1 - tl < 1 ? NTA - 1 - tl : 1);
      if (tl == NTA - 1) patch_f(tl);   // the only tile that holds the last row of F
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      if (tl + 2 < NTA) issue_a(tl + 2);
      const uint32_t bo = (uint32_t)((tl % 3) * G4_PA_BUF);
      u32x4 xa[4][2], ffr[2];
      u32x2 fl[2], fh[2];
      g4_read_a<0>(xa, ar0 + bo, ar1 + bo);
      if constexpr (NT) {
        g4_rd128<0>(ffr[0], fr0 + bo);
        g4_rd128<0>(ffr[1], fr1 + bo);
      } else {
        g4_rdtr<0>(fl[0], fr0 + bo);
        g4_rdtr<512>(fh[0], fr0 + bo);
        g4_rdtr<4096>(fl[1], fr0 + bo);
        g4_rdtr<4096 + 512>(fh[1], fr0 + bo);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (!NT) ffr[0] = join2(fl[0], fh[0]), ffr[1] = join2(fl[1], fh[1]);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) hacc[0][mt] = G4_MFMA(ffr[ks], xa[mt][ks], hacc[0][mt]);
      __builtin_amdgcn_sched_barrier(0);
      g4_read_a<1>(xa, ar0 + bo, ar1 + bo);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) hacc[1][mt] = G4_MFMA(ffr[ks], xa[mt][ks], hacc[1][mt]);
      __builtin_amdgcn_sched_barrier(0);
    }
    // H^T tile (rows = rank 4 g + j of rank tile wc, column = token r16) -> bf16 -> the k-contiguous image the extension reads
#pragma unroll
    for (int mh = 0; mh < 2; ++mh)
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const int lr = wr * 64 + mt * 16 + r16;
        const int q = wc * 2 + (g >> 1);
        char* dst = smem + G4_HIMG + mh * G4_HALF + lr * 128 + ((q ^ ((lr >> 1) & 7)) * 16) + (g & 1) * 8;
        f32x4 v = hacc[mh][mt];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (wc * 16 + 4 * g + j < p.r) ? v[j] * p.hscale : 0.f;   // ranks >= r: exact zeros
        *(u32x2*)dst = (u32x2){G4_PACK(v[0], v[1]), G4_PACK(v[2], v[3])};
      }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();      // every read of the projection buffers is done: the ring belongs to the main loop
    __builtin_amdgcn_sched_barrier(0);
    // the main loop starts over at k = 0
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
#pragma unroll
      for (int ii = 0; ii < 2; ++ii) pA[hh][ii] = p.A + a_row(hh, c_lr[ii]) * p.lda + 8 * c_q[ii];
  }

  // ------------------------------------------------------------------ fragment addresses (per lane)
  const uint32_t base = lds_addr(smem);
  const int fsw = (r16 >> 1) & 7;
  const int ch0 = (fsw & 4) | (g ^ (fsw & 3));                  // physical chunk of k-step 0 (k-step 1: ^ 4)
  uint32_t a_off[2], b_off[2];                                  // [ks] (NT) / [nt] (NN); buffer bit toggled per K-tile
  a_off[0] = base + (uint32_t)((wr * 64 + r16) * 128 + ch0 * 16);
  a_off[1] = base + (uint32_t)((wr * 64 + r16) * 128 + (ch0 ^ 4) * 16);
  if constexpr (NT) {
    b_off[0] = base + (uint32_t)(G4_OFF_B0 + (wc * 32 + r16) * 128 + ch0 * 16);
    b_off[1] = base + (uint32_t)(G4_OFF_B0 + (wc * 32 + r16) * 128 + (ch0 ^ 4) * 16);
  } else {
    const int qq = r16 >> 2, pp = r16 & 3;
    const int f = (qq | ((g & 1) << 2)) << 1;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int chunk = wc * 4 + nt * 2 + (pp >> 1);
      b_off[nt] = base + (uint32_t)(G4_OFF_B0 + (8 * g + qq) * 256 + ((chunk ^ f) * 16) + 8 * (pp & 1));
    }
  }

  f32x4 acc[2][4][2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int d = 0; d < 2; ++d) acc[a][b][c][d] = (f32x4){0.f, 0.f, 0.f, 0.f};
  u32x4 af[4][2];           // [mt][ks]      x fragments of the current row half
  u32x4 bf[2][2][2];        // [nh][nt][ks]  W fragments of both column halves (k-contiguous image)
  u32x2 bl[2][2][2], bh[2][2][2];   // the same from the k-major image: low / high four k of every fragment

  auto read_a = [&](auto mh_c) { g4_read_a<decltype(mh_c)::value>(af, a_off[0], a_off[1]); };
  auto read_b = [&](auto nh_c) {
    constexpr int NH = decltype(nh_c)::value;
    if constexpr (NT) g4_read_b_nt<NH>(bf[NH], b_off[0], b_off[1]);
    else g4_read_b_nn<NH>(bl[NH], bh[NH], b_off[0], b_off[1]);
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;

  // one phase of K-tile `tile`: fragment reads of the quadrant, DMA of half-tile P + 6, counted wait, barrier, 16 MFMAs, barrier
  auto phase = [&](auto ph_c, auto tail_c, int tile) {
    constexpr int PH = decltype(ph_c)::value;
    constexpr bool TAIL = decltype(tail_c)::value;
    constexpr int MH = PH >= 2 ? 1 : 0;
    constexpr int NH = (PH == 1 || PH == 2) ? 1 : 0;
    if constexpr (PH == 0) {
      read_b(I0{});
      __builtin_amdgcn_sched_barrier(0);
      read_a(I0{});
    } else if constexpr (PH == 1) {
      read_b(I1{});
    } else if constexpr (PH == 2) {
      read_a(I1{});
    }
    __builtin_amdgcn_sched_barrier(0);
    const int P = 4 * tile + PH;
    const int h = P + 6;
    if (!TAIL || h < H) {
      if constexpr (PH == 0) issue(KB1{}, h >> 2);
      else if constexpr (PH == 1) issue(KA1{}, h >> 2);
      else if constexpr (PH == 2) issue(KA0{}, h >> 2);
      else issue(KB0{}, h >> 2);
    }
    if constexpr (!TAIL) {
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
    } else {
      int newer = H - 3 - P;
      newer = newer < 0 ? 0 : (newer > 4 ? 4 : newer);
      wait_groups<2>(newer);
    }
    __builtin_amdgcn_s_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          u32x4 wf;
          if constexpr (NT) wf = bf[NH][nt][ks];
          else wf = join2(bl[NH][nt][ks], bh[NH][nt][ks]);
          acc[MH][mt][NH][nt] = G4_MFMA(wf, af[mt][ks], acc[MH][mt][NH][nt]);
        }
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (PH == 3) {   // next K-tile: the other buffer
      a_off[0] ^= G4_BUF, a_off[1] ^= G4_BUF, b_off[0] ^= G4_BUF, b_off[1] ^= G4_BUF;
    }
  };
  using T0 = std::integral_constant<bool, false>;
  using T1 = std::integral_constant<bool, true>;
  using P0 = std::integral_constant<int, 0>;
  using P1 = std::integral_constant<int, 1>;
  using P2 = std::integral_constant<int, 2>;
  using P3 = std::integral_constant<int, 3>;

  // ------------------------------------------------------------------ prologue: half-tiles 0 .. 5 (of this block's K range)
  if (kt0 & 1) a_off[0] ^= G4_BUF, a_off[1] ^= G4_BUF, b_off[0] ^= G4_BUF, b_off[1] ^= G4_BUF;
  issue(KA0{}, kt0), issue(KB0{}, kt0), issue(KB1{}, kt0), issue(KA1{}, kt0);
  if (NTL - kt0 > 1) issue(KA0{}, kt0 + 1), issue(KB0{}, kt0 + 1);
  wait_groups<2>(NTL - kt0 > 1 ? 4 : 2);     // A0, B0 of the first K-tile have landed (this wave's pieces)
  __builtin_amdgcn_s_barrier();        // ... everyone's
  __builtin_amdgcn_sched_barrier(0);
  if (wr == 1) __builtin_amdgcn_s_barrier();   // the second wave row runs one barrier behind the first
  __builtin_amdgcn_sched_barrier(0);

  int tile = kt0;
#pragma unroll 1
  for (; tile < NTL - 2; ++tile) {
    phase(P0{}, T0{}, tile);
    phase(P1{}, T0{}, tile);
    phase(P2{}, T0{}, tile);
    phase(P3{}, T0{}, tile);
  }
#pragma unroll 1
  for (; tile < NTL - 1; ++tile) {
    phase(P0{}, T1{}, tile);
    phase(P1{}, T1{}, tile);
    phase(P2{}, T1{}, tile);
    phase(P3{}, T1{}, tile);
  }
  // the last K-tile, outside the loop (gemm4h: the extension tile, with its operand switch and the end-of-buffer patch)
  if (tile < NTL) {
    if constexpr (HF) {
      if (tile == NTL - 1) {   // the extension tile: A fragments come from the projected tile
        a_off[0] = base + (uint32_t)(G4_HIMG + (wr * 64 + r16) * 128 + ch0 * 16);
        a_off[1] = base + (uint32_t)(G4_HIMG + (wr * 64 + r16) * 128 + (ch0 ^ 4) * 16);
        if constexpr (NT) {
          if (p.ldb2 != 64) {
            // B2 = raw A: rewrite the pieces that crossed the end of the buffer (every DMA has been issued by now).  Two
            // barriers: the wave rows are one barrier apart, and the other row's patch must be visible before the reads
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int hh = 0; hh < 2; ++hh)
#pragma unroll
              for (int ii = 0; ii < 2; ++ii) {
                const int kk = 8 * c_q[ii];
                const int64_t eoff = (int64_t)b_col_nt(hh, c_lr[ii]) * p.ldb2 + kk;
                if (kk < p.k2e && eoff + 8 > (int64_t)N * p.ldb2) {
                  u32x4 v;
                  bf16_t* e = (bf16_t*)&v;
#pragma unroll
                  for (int j = 0; j < 8; ++j) e[j] = (kk + j < p.k2e) ? p.B2[eoff + j] : (bf16_t)0.f;
                  *(u32x4*)(smem + (tile & 1) * G4_BUF + (hh ? G4_OFF_B1 : G4_OFF_B0) + (2 * w + ii) * 1024 + lane * 16) = v;
                }
              }
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
    }
    phase(P0{}, T1{}, tile);
    phase(P1{}, T1{}, tile);
    phase(P2{}, T1{}, tile);
    phase(P3{}, T1{}, tile);
  }
  if (wr == 0) __builtin_amdgcn_s_barrier();   // catch up: every wave has passed its last fragment read
  __builtin_amdgcn_sched_barrier(0);

  // ------------------------------------------------------------------ epilogue
  // acc[mh][mt][nh][nt][j] = C[row = 128 wr + 64 mh + 16 mt + r16][col = 64 wc + 32 nh + 16 nt + 4 g + j]
  float* sc = (float*)(smem + w * G4_SCR);
  const bool nts = p.nt_store != 0;
#pragma unroll
  for (int mh = 0; mh < 2; ++mh)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
      for (int nh = 0; nh < 2; ++nh)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) *(f32x4*)(sc + r16 * G4_SCR_LD + nh * 32 + nt * 16 + 4 * g) = acc[mh][mt][nh][nt];
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int pass = 0; pass < 2; ++pass) {
        const int r = pass * 8 + (lane >> 3), c = (lane & 7) * 8;
        const int64_t grow = m0 + wr * 128 + mh * 64 + mt * 16 + r;
        const int gcol = n0 + wc * 64 + c;
        if (grow < M && gcol < N) {
          float v[8];
          const f32x4 t0 = *(const f32x4*)(sc + r * G4_SCR_LD + c), t1 = *(const f32x4*)(sc + r * G4_SCR_LD + c + 4);
          if constexpr (SK) {
            // split-K: the fp32 sum of this block's K range, row-major [split][M][N] (256-byte row segments); alpha, beta, bias and
            // the rounding to bf16 happen once, in gemm4_splitk_reduce_kernel
            float* pd = p.partials + ((size_t)split * (size_t)M + (size_t)grow) * (size_t)N + gcol;
            *(f32x4*)pd = t0, *(f32x4*)(pd + 4) = t1;
            continue;
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = t0[j] * p.alpha, v[4 + j] = t1[j] * p.alpha;
          bf16_t* dst = p.C + grow * p.ldc + gcol;
          if (p.beta != 0.f) {
            const u32x4 old = *(const u32x4*)dst;
            const G4_T* o = (const G4_T*)&old;
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] += p.beta * (float)o[j];
          }
          if (p.bias) {
            const u32x4 bv = *(const u32x4*)(p.bias + gcol);
            const G4_T* b = (const G4_T*)&bv;
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] += (float)b[j];
          }
          u32x4 pk;
#pragma unroll
          for (int j = 0; j < 4; ++j) pk[j] = G4_PACK(v[2 * j], v[2 * j + 1]);
          if (nts) asm volatile("global_store_dwordx4 %0, %1, off nt\n\ts_nop 1" ::"v"(dst), "v"(pk) : "memory");
          else *(u32x4*)dst = pk;
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
  // gemm4h: the saved copy of the projection (h_save / dh: [M, 64], column 63 <- 1.0 when free -- the dbias column of the
  // weight-gradient kernels), written once per row panel, after the C stores
  if constexpr (HF) {
    if (n0 == 0 && p.Hout) {
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int idx = it * G4_THREADS + t;
        const int half = idx >> 10, lr = (idx >> 3) & 127, pc = idx & 7;
        const int q = pc ^ ((lr >> 1) & 7);
        const int64_t grow = m0 + (lr >> 6) * 128 + half * 64 + (lr & 63);
        if (grow < M) {
          u32x4 v = *(const u32x4*)(smem + G4_HIMG + half * G4_HALF + lr * 128 + pc * 16);
          if (q == 7 && p.r < 64) v[3] = (v[3] & 0xffffu) | (G4_ONE << 16);
          *(u32x4*)(p.Hout + grow * 64 + q * 8) = v;
        }
      }
    }
  }
}

// C = alpha * sum_s partial[s] + beta * C + bias, 8 columns per thread (N % 8 == 0), splits added in order (deterministic)
__global__ __launch_bounds__(256) void G4_REDUCE(const float* __restrict__ part, int splits, int64_t M, int N,
                                                                  G4_T* C, int64_t ldc, const G4_T* bias, float alpha, float beta) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int n8 = N / 8;
  if (idx >= M * n8) return;
  const int64_t row = idx / n8;
  const int col = (int)(idx % n8) * 8;
  const float* src = part + row * N + col;
  f32x4 a0 = __builtin_nontemporal_load((const f32x4*)src), a1 = __builtin_nontemporal_load((const f32x4*)(src + 4));
  for (int s = 1; s < splits; ++s) {
    const float* q = src + (size_t)s * (size_t)M * (size_t)N;
    a0 += __builtin_nontemporal_load((const f32x4*)q), a1 += __builtin_nontemporal_load((const f32x4*)(q + 4));
  }
  float v[8] = {a0[0] * alpha, a0[1] * alpha, a0[2] * alpha, a0[3] * alpha, a1[0] * alpha, a1[1] * alpha, a1[2] * alpha, a1[3] * alpha};
  G4_T* dst = C + row * ldc + col;
  if (beta != 0.f) {
    const u32x4 old = *(const u32x4*)dst;
    const G4_T* o = (const G4_T*)&old;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] += beta * (float)o[j];
  }
  if (bias) {
    const u32x4 bv = *(const u32x4*)(bias + col);
    const G4_T* b = (const G4_T*)&bv;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] += (float)b[j];
  }
  u32x4 pk;
#pragma unroll
  for (int j = 0; j < 4; ++j) pk[j] = G4_PACK(v[2 * j], v[2 * j + 1]);
  *(u32x4*)dst = pk;
}

