// Fused wide-rank chain (64 < r <= 256, bf16 / f16): the low-rank term of a layer in ONE pass over the token rows.
//
//   H = rn(hscale * X . F1)                   [64 tokens x r_pad] per workgroup, kept in LDS (copied to Hsave [M, r])
//   Y = beta * Y + yscale * H . F2 + bias     Y written once, with the rounding of the generic GEMM epilogue
//
// forward       X = x,  F1 = A,   F2 = B,   hscale = 1, yscale = s   (h_save = rn(x . A), the wide-rank contract)
// data gradient X = dY, F1 = B^T, F2 = A^T, hscale = s, yscale = 1   (dh = rn(s dY . B^T) kept for the weight pass,
//                                                                      dX = beta dX + dh . A^T)
// The projection of a token tile never leaves the chip: the generic composition writes [M, r] to HBM and reads it back.
//
// The factors are first packed (one small launch, wide_pack_kernel) into k-contiguous, zero-padded images in the caller's
// workspace: F1T [r_pad][D1] (row c = column c of H) and F2T [D2][r_pad] (row n = output column n), so that every operand
// tile is staged with 16-byte loads and the padding columns r .. r_pad - 1 contribute exact zeros.
//
// Workgroup = 256 threads (4 waves), 64 tokens.  LDS: 64 KiB static, two workgroups per CU.
//   phase 1 (K = D1 in 64-wide steps): [0, 32K) F1 image [r_pad][64], [32K, 40K) X image [64][64];
//            H tiles (2 token halves x r_pad / 32 column tiles) dealt round-robin to the waves, <= 4 per wave;
//   phase 2 (per 64 output columns): [0, 32K) H as r_pad / 64 panels [64][64], [32K, 64K) F2 panels [64][64], reused as
//            the epilogue scratch once the panel's products are done; wave (wm, wn) owns a 32 x 32 output tile.
//
// Ragged widths (RAG: D1 or D2 not a multiple of 8, even r in [2, 256]): a token row of X starts at any 2-byte offset.
// Each thread still stages 8 consecutive elements of one row: it reads the one or two aligned 16-byte pieces that hold
// them through a buffer descriptor limited to the workgroup's own rows (so the last piece of the tensor reads zeros past
// its end), shifts them into place in registers and zeroes the columns >= D1; the LDS image is then written at its
// natural alignment, exactly as in the aligned kernel.  F1T rows are padded to D1p = ceil8(D1) by the pack.  Y is
// written element by element (2-byte stores): no byte of a token row is written by another workgroup, whatever D2.
// The ragged kernel also takes 2 <= r <= 64 (r_pad = 64) for a layer's low-rank accumulator term, which saves no H.
#include "chain_wide_tile.hpp"

namespace sow {

struct WidePack {
  const void* src;
  int64_t lds;
  void* dst;
  int R, C;      // dst [R][C]
  int rv, cv;    // dst element (i, j) is a source element when i < rv and j < cv, else 0
  int trans;     // source element = trans ? src[j][i] : src[i][j]
};
struct WidePackParams {
  WidePack job[2];
  int64_t n0, n;   // elements of job 0, of both
};

template <typename T> __global__ __launch_bounds__(256) void wide_pack_kernel(const WidePackParams p) {
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.n) return;
  const WidePack& J = p.job[i >= p.n0 ? 1 : 0];
  if (i >= p.n0) i -= p.n0;
  const int r = (int)(i / J.C), c = (int)(i % J.C);
  T v = from_f32<T>(0.f);
  if (r < J.rv && c < J.cv) v = J.trans ? ((const T*)J.src)[(int64_t)c * J.lds + r] : ((const T*)J.src)[(int64_t)r * J.lds + c];
  ((T*)J.dst)[i] = v;
}

struct WideParams {
  const void* X;
  void* Y;
  const void* F1T;   // [r_pad][ldf1t]
  const void* F2T;   // [D2][r_pad]
  void* Hsave;       // [M][r] or nullptr
  const void* bias;  // [D2] or nullptr
  int64_t M;
  int D1, D2, r, r_pad, ldf1t;
  float hscale, yscale, beta;
  int nt_store;
};

template <typename T, bool RAG> __global__ __launch_bounds__(256, 2) void chain_wide_kernel(const WideParams p) {
  __shared__ __attribute__((aligned(16))) char smem[CW_LDS];
  char* big = smem;              // F1 image, then the H panels
  char* small = smem + 32768;    // X image, then the F2 panels / epilogue scratch

  const int t = threadIdx.x, lane = t & 63, w = t >> 6, li = lane & 31;
  const int64_t t0 = (int64_t)blockIdx.x * 64;
  const int r_pad = p.r_pad, ntiles = 2 * (r_pad / 32);

  // ---- phase 1: H = X . F1 (chain_wide_tile.hpp) ------------------------------------------------------------
  f32x16 acc[4];
  cw_phase1<T, RAG>(acc, big, small, (const T*)p.X, (const T*)p.F1T, p.M, t0, p.D1, p.ldf1t, r_pad);

  // ---- H (rounded once) -> LDS panels, then Hsave ---------------------------------------------------------
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = w + 4 * i;
    if (j < ntiles) {
      const int c = (j >> 1) * 32 + li;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg)
        *(T*)(big + cw_panel_off<T>((j & 1) * 32 + acc_row(reg, lane), c)) = from_f32<T>(p.hscale * acc[i][reg]);
    }
  }
  __syncthreads();
  if (p.Hsave) {
    const int pairs = p.r >> 1;
    T* H = (T*)p.Hsave;
    for (int idx = t; idx < 64 * pairs; idx += 256) {
      const int row = idx / pairs, c = 2 * (idx % pairs);
      const int64_t gt = t0 + row;
      if (gt < p.M) *(uint32_t*)(H + gt * p.r + c) = *(const uint32_t*)(big + cw_panel_off<T>(row, c));
    }
  }

  // ---- phase 2: Y = beta * Y + yscale * H . F2 + bias, 64 output columns at a time ------------------------
  cw_phase2<T, !RAG>(big, small, (const T*)p.F2T, (T*)p.Y, (const T*)p.bias, p.M, t0, p.D2, r_pad, p.yscale, p.beta,
                     p.nt_store != 0);
}

bool chain_wide_shape_ok(int r, int d1, int d2, int dtype) {
  return (dtype == SOW_BF16 || dtype == SOW_F16) && r > 64 && r <= 256 && r % 2 == 0 && d1 % 8 == 0 && d2 % 8 == 0;
}

bool ragged_shape_ok(int r, int d1, int d2, int dtype) {
  return (dtype == SOW_BF16 || dtype == SOW_F16) && r >= 2 && r <= 256 && r % 2 == 0 && (d1 % 8 != 0 || d2 % 8 != 0) &&
         d1 > 0 && d2 > 0 && d1 <= (1 << 23) && d2 <= (1 << 23);
}

// F1T [r_pad][ceil8(D1)] + F2T [D2][r_pad], D1 / D2 = d_in / d_out in either order
size_t chain_wide_pack_bytes(int r, int d_in, int d_out) {
  const size_t r_pad = (size_t)(r + 63) / 64 * 64, p_in = (size_t)(d_in + 7) / 8 * 8, p_out = (size_t)(d_out + 7) / 8 * 8;
  return ((r_pad * p_in * 2 + 255) & ~(size_t)255) + ((r_pad * p_out * 2 + 255) & ~(size_t)255);
}

int launch_chain_wide(const WideArgs& a, int dtype, hipStream_t stream) {
  const bool rag = a.D1 % 8 != 0 || a.D2 % 8 != 0;
  if (!(rag ? ragged_shape_ok(a.r, a.D1, a.D2, dtype) : chain_wide_shape_ok(a.r, a.D1, a.D2, dtype))) return SOW_ERR_UNSUPPORTED;
  if ((rag && a.r <= 64 && a.Hsave) || !al16p(a.X) || !al16p(a.Y) || (a.bias && !al16p(a.bias)) || !al16p(a.pack) ||
      (a.Hsave && (reinterpret_cast<uintptr_t>(a.Hsave) & 3)) || !a.pack ||
      a.pack_bytes < chain_wide_pack_bytes(a.r, a.D1, a.D2))
    return SOW_ERR_UNSUPPORTED;
  if (a.M <= 0) return SOW_OK;
  if (ceil_div(a.M, 64) > 0x7fffffff) return SOW_ERR_SHAPE;
  const int r_pad = (a.r + 63) / 64 * 64, d1p = (a.D1 + 7) / 8 * 8;
  char* f1t = (char*)a.pack;
  char* f2t = f1t + (((size_t)r_pad * d1p * 2 + 255) & ~(size_t)255);
  // F1T [r_pad][d1p]: column c of F1 (forward: A [D1][r], transposed; data gradient: B [r][D1], as stored)
  // F2T [D2][r_pad]: column n of F2 (forward: B [r][D2], transposed; data gradient: A [D2][r], as stored)
  WidePackParams pk{};
  pk.job[0] = WidePack{a.F1, a.ldf1, f1t, r_pad, d1p, a.r, a.D1, a.bwd ? 0 : 1};
  pk.job[1] = WidePack{a.F2, a.ldf2, f2t, a.D2, r_pad, a.D2, a.r, a.bwd ? 0 : 1};
  pk.n0 = (int64_t)r_pad * d1p;
  pk.n = pk.n0 + (int64_t)a.D2 * r_pad;
  WideParams p{};
  p.X = a.X, p.Y = a.Y, p.F1T = f1t, p.F2T = f2t, p.Hsave = a.Hsave, p.bias = a.bias;
  p.M = a.M, p.D1 = a.D1, p.D2 = a.D2, p.r = a.r, p.r_pad = r_pad, p.ldf1t = d1p;
  p.hscale = a.hscale, p.yscale = a.yscale, p.beta = a.beta;
  p.nt_store = SOW_GEMM_NT(a.M) ? 1 : 0;
  const dim3 pgrid((unsigned)((pk.n + 255) / 256)), grid((unsigned)ceil_div(a.M, 64));
  if (dtype == SOW_BF16) {
    hipLaunchKernelGGL(wide_pack_kernel<bf16_t>, pgrid, dim3(256), 0, stream, pk);
    if (rag) hipLaunchKernelGGL((chain_wide_kernel<bf16_t, true>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((chain_wide_kernel<bf16_t, false>), grid, dim3(256), 0, stream, p);
  } else {
    hipLaunchKernelGGL(wide_pack_kernel<f16_t>, pgrid, dim3(256), 0, stream, pk);
    if (rag) hipLaunchKernelGGL((chain_wide_kernel<f16_t, true>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((chain_wide_kernel<f16_t, false>), grid, dim3(256), 0, stream, p);
  }
  SOW_CHECK_LAUNCH();
  return SOW_OK;
}

}  // namespace sow
