// Fused low-rank-accumulator chain (bf16 / f16): the accumulator term AND the live term of a layer in ONE pass over the
// token rows -- the two factor pairs side by side in one chain (SOW_FUSE_ACC, include/sow_amd.h).
//
//   H = X . [Fa1 | Fl1]                        [64 tokens x r_pad] per workgroup, fp32, r_pad = ceil64(r_acc + r_live)
//   h = rn(s_c * H)                            s_c = 1 for the accumulator columns c < r_acc, `scale` for the live columns;
//                                              kept in LDS; the live columns leave as Hsave [M, 64] (the r <= 64 contract)
//   Y = rn(h . [Fa2 ; Fl2] + bias)             one fp32 accumulation over the r_pad columns, one rounding, Y written once
//
// forward       X = x,  Fa1 = Q,   Fl1 = A,   Fa2 = R,   Fl2 = B     (h_save = rn(scale x A), y = rn(xQ.R + h.B + bias))
// data gradient X = dY, Fa1 = R^T, Fl1 = B^T, Fa2 = Q^T, Fl2 = A^T   (dh = rn(scale dY B^T), dX = rn(dY R^T . Q^T + dh . A^T))
// The values rounded in the middle are the ones the two-pass path rounds (chain2 / chain_wide for the accumulator with scale
// 1, chain2 for the live term); what the fused pass drops is the rounding of the accumulator term's Y between the launches.
// No atomics, a fixed summation order: a repeated call gives the same bits.
//
// The four factors are first packed (one small launch, wide_acc_pack_kernel) into the k-contiguous, zero-padded images
// chain_wide.hip describes: F1T [r_pad][D1] (row c = column c of H: rows [0, r_acc) from Fa1, [r_acc, r_acc + r_live) from
// Fl1) and F2T [D2][r_pad] (row n = output column n, the matching columns).  Padding is exact zeros, and the kernel also
// masks the padding columns of h, so that a non-finite X cannot reach Y through 0 * inf of a column that does not exist.
//
// Workgroup = 256 threads (4 waves), 64 tokens; LDS: 64 KiB static, two workgroups per CU; the tile code is the one
// chain_wide_kernel<T, false> runs (chain_wide_tile.hpp: phase 1 over K = D1 in 64-wide steps, phase 2 per 64 output columns,
// wave_store_tiles).
// Hsave rows are written whole: 8 lanes x 16 bytes = one 128-byte row, streaming stores (the weight-gradient pass reads them
// next).  The accumulator columns of h are never written to memory.
#include "chain_wide_tile.hpp"
#include "lds_dma.hpp"

namespace sow {

struct WideAccParams {
  const void* X;
  void* Y;
  const void* F1T;   // [r_pad][D1]
  const void* F2T;   // [D2][r_pad]
  void* Hsave;       // [M][64] or nullptr
  const void* bias;  // [D2] or nullptr
  int64_t M;
  int D1, D2, r_acc, r_live, r_pad;
  float scale;
  int nt_store;
};

template <typename T> __global__ __launch_bounds__(256, 2) void chain_wide_acc_kernel(const WideAccParams p) {
  __shared__ __attribute__((aligned(16))) char smem[CW_LDS];
  char* big = smem;              // F1 image, then the H panels
  char* small = smem + 32768;    // X image, then the F2 panels / epilogue scratch

  const int t = threadIdx.x, lane = t & 63, w = t >> 6, li = lane & 31;
  const int64_t t0 = (int64_t)blockIdx.x * 64;
  const int r_pad = p.r_pad, ntiles = 2 * (r_pad / 32), r_tot = p.r_acc + p.r_live;

  // ---- phase 1: H = X . [Fa1 | Fl1] (chain_wide_tile.hpp) ---------------------------------------------------------
  f32x16 acc[4];
  cw_phase1<T, false>(acc, big, small, (const T*)p.X, (const T*)p.F1T, p.M, t0, p.D1, p.D1, r_pad);

  // ---- h = rn(s_c * H), s_c per column, padding columns zero -> LDS panels ------------------------------------------
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = w + 4 * i;
    if (j < ntiles) {
      const int c = (j >> 1) * 32 + li;
      const float s = c < p.r_acc ? 1.f : p.scale;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg)
        *(T*)(big + cw_panel_off<T>((j & 1) * 32 + acc_row(reg, lane), c)) = from_f32<T>(c < r_tot ? s * acc[i][reg] : 0.f);
    }
  }
  __syncthreads();
  // ---- the live columns -> Hsave [M][64]: data below r_live, zeros above, 1.0 in column 63 when r_live < 64 (the dbias
  // column of the weight-gradient kernels); 8 lanes write one whole 128-byte row
  if (p.Hsave) {
    T* H = (T*)p.Hsave;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int row = pass * 32 + (t >> 3), c0 = (t & 7) * 8;
      const int64_t gt = t0 + row;
      u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = c0 + 2 * q;   // r_acc and r_live are even: a pair is data or padding as a whole, and 4-byte aligned
        if (c < p.r_live) v[q] = *(const uint32_t*)(big + cw_panel_off<T>(row, p.r_acc + c));
      }
      if (c0 == 56 && p.r_live < 64) v[3] = (v[3] & 0xffffu) | (DT<T>::one_bits << 16);
      if (gt < p.M) store_b128_nt(H + gt * 64 + c0, v);   // (carries the wait states a 16-byte store needs before v is rewritten)
    }
  }

  // ---- phase 2: Y = rn(h . [Fa2 ; Fl2] + bias), 64 output columns at a time, one rounding ---------------------------
  cw_phase2<T, true>(big, small, (const T*)p.F2T, (T*)p.Y, (const T*)p.bias, p.M, t0, p.D2, r_pad, 1.f, 0.f, p.nt_store != 0);
}

// The admitted set of SOW_FUSE_ACC (include/sow_amd.h), a pure function of the shape and the compute dtype
bool fused_acc_shape_ok(int r_live, int r_acc, int d_in, int d_out, int dtype) {
  return (dtype == SOW_BF16 || dtype == SOW_F16) && r_live >= 2 && r_live <= 64 && r_live % 2 == 0 && r_acc >= 2 &&
         r_acc % 2 == 0 && r_acc + r_live <= 256 && d_in > 0 && d_out > 0 && d_in % 8 == 0 && d_out % 8 == 0;
}

int launch_chain_wide_acc(const WideAccArgs& a, int dtype, hipStream_t stream) {
  if (!fused_acc_shape_ok(a.r_live, a.r_acc, a.D1, a.D2, dtype)) return SOW_ERR_UNSUPPORTED;
  if (!al16p(a.X) || !al16p(a.Y) || !al16p(a.bias) || !al16p(a.Hsave) || !a.pack || !al16p(a.pack) ||
      a.pack_bytes < chain_wide_pack_bytes(a.r_acc + a.r_live, a.D1, a.D2))
    return SOW_ERR_UNSUPPORTED;
  if (a.M <= 0) return SOW_OK;
  if (ceil_div(a.M, 64) > 0x7fffffff) return SOW_ERR_SHAPE;
  const int r_tot = a.r_acc + a.r_live, r_pad = (r_tot + 63) / 64 * 64;
  const WideAccPackParams pk = wide_acc_pack_params(a);
  void *f1t = pk.f1t, *f2t = pk.f2t;
  WideAccParams p{};
  p.X = a.X, p.Y = a.Y, p.F1T = f1t, p.F2T = f2t, p.Hsave = a.Hsave, p.bias = a.bias;
  p.M = a.M, p.D1 = a.D1, p.D2 = a.D2, p.r_acc = a.r_acc, p.r_live = a.r_live, p.r_pad = r_pad;
  p.scale = a.scale;
  p.nt_store = SOW_GEMM_NT(a.M) ? 1 : 0;
  const dim3 pgrid((unsigned)((pk.n + 255) / 256)), grid((unsigned)ceil_div(a.M, 64));
  if (dtype == SOW_BF16) {
    hipLaunchKernelGGL(wide_acc_pack_kernel<bf16_t>, pgrid, dim3(256), 0, stream, pk);
    hipLaunchKernelGGL(chain_wide_acc_kernel<bf16_t>, grid, dim3(256), 0, stream, p);
  } else {
    hipLaunchKernelGGL(wide_acc_pack_kernel<f16_t>, pgrid, dim3(256), 0, stream, pk);
    hipLaunchKernelGGL(chain_wide_acc_kernel<f16_t>, grid, dim3(256), 0, stream, p);
  }
  SOW_CHECK_LAUNCH();
  return SOW_OK;
}

}  // namespace sow
