// Fused low-rank-accumulator chain past 256 columns (bf16 / f16): the pass of chain_wide_acc.hip for 256 < r_acc + r_live <=
// 960, the H columns of ONE chain computed in groups of 256 and kept side by side in dynamic LDS (SOW_FUSE_ACC_DEEP,
// include/sow_amd.h).  With r_pad = ceil64(r_acc + r_live) and G = ceil(r_pad / 256) column groups:
//
//   H_g = X . F1[:, 256 g ..]                  [64 tokens x min(256, r_pad - 256 g)] per group, fp32, K = D1; the token
//                                              block's X tile is read once per group (64 x D1 elements: the re-reads hit L2)
//   h   = rn(s_c * H)                          s_c = 1 for the accumulator columns c < r_acc, `scale` for the live columns,
//                                              padding columns c >= r_acc + r_live exact zeros; kept in LDS as r_pad / 64
//                                              panels; the live columns leave as Hsave [M, 64] (the r <= 64 contract)
//   Y   = rn(h . [Fa2 ; Fl2] + bias)           one fp32 accumulation over the panels in ascending order, ascending k inside a
//                                              panel, the bias added in fp32, ONE rounding, Y written once (beta = 0)
//
// forward and data gradient map onto X / F1 / F2 as in chain_wide_acc.hip, and the factors come in the same pack
// (wide_acc_pack_params: F1T [r_pad][D1], F2T [D2][r_pad], exact zeros in the padding): one pack launch and one kernel launch
// per direction.  No atomics, a fixed order: a repeated call gives the same bits.  The accumulator columns of h never reach
// memory.  A non-finite X[t, k] reaches row t only: the padding columns of h are masked after the product.
//
// Workgroup = 256 threads (4 waves), 64 tokens.  Dynamic LDS (deep_acc_lds_bytes):
//   [ H panels: r_pad x 128 B ][ stage, 40 KiB: the F1 image of a group (32 KiB) and the X image (8 KiB) in phase 1; in phase
//   2 four F2 panels of 8 KiB at a time, then the epilogue scratch (18 KiB) ]
// r_pad = 320: 40 + 40 = 80 KiB, two workgroups per CU; r_pad = 960: 120 + 40 = exactly 160 KiB, 15 panels, one per CU.
// Hsave is written after the last group and a barrier: the live columns [r_acc, r_acc + r_live) may straddle a group boundary.
#include <type_traits>

#include "chain_wide_tile.hpp"
#include "lds_dma.hpp"

namespace sow {

constexpr size_t DEEP_MAX_LDS = 160 * 1024;
constexpr int DEEP_STAGE = 40960, DEEP_XOFF = 32768, DEEP_GROUP = 256, DEEP_MAX_TOT = 960;
static_assert(CW_MAXP >= DEEP_MAX_TOT / 64, "the panel table must hold every panel of the widest chain");
static_assert((size_t)DEEP_MAX_TOT * 128 + DEEP_STAGE == DEEP_MAX_LDS, "the widest admitted chain plans exactly the LDS limit");

struct DeepAccParams {
  CwPanels pan;      // the r_pad / 64 panels in order, each with its 64-column slice of F2T [D2][r_pad]
  const void* X;
  void* Y;
  const void* F1T;   // [r_pad][D1]
  void* Hsave;       // [M][64] or nullptr
  const void* bias;  // [D2] or nullptr
  int64_t M;
  int D1, D2, r_acc, r_live, r_pad;
  float scale;
  int nt_store;
};
// The parameter block is read where it lies, in the kernel-argument segment (as chain_shared_acc_kernel reads its own): the
// entry of panel q is then a scalar load at a uniform index.  This holds only while DeepAccParams is the kernel's FIRST
// explicit argument: put no argument before it, and keep the struct plain data.
static_assert(std::is_trivially_copyable<DeepAccParams>::value && std::is_standard_layout<DeepAccParams>::value,
              "DeepAccParams is read from the kernel-argument segment as it is laid out on the host");
#define DEEP_KARG __attribute__((address_space(4)))
template <typename T> __global__ __launch_bounds__(256, 2) void chain_deep_acc_kernel(const DeepAccParams) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const DeepAccParams DEEP_KARG& p = *(const DeepAccParams DEEP_KARG*)__builtin_amdgcn_kernarg_segment_ptr();
  const int r_pad = p.r_pad, r_acc = p.r_acc, r_live = p.r_live, r_tot = r_acc + r_live;
  char* stage = smem + r_pad * 128;
  const int64_t t0 = (int64_t)blockIdx.x * 64;

  // ---- phase 1 per column group: H_g = X . F1[:, 256 g ..] (chain_wide_tile.hpp), the F1 and X images in the stage ------
  for (int c0 = 0; c0 < r_pad; c0 += DEEP_GROUP) {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));   // keeps the per-lane address arithmetic inside the iteration (as chain_shared_acc_kernel does)
    const int lane = t & 63, w = t >> 6, li = lane & 31;
    const int gw = r_pad - c0 < DEEP_GROUP ? r_pad - c0 : DEEP_GROUP, ntiles = 2 * (gw / 32);
    f32x16 acc[4];
    cw_phase1_at<T, false>(acc, stage, stage + DEEP_XOFF, (const T*)p.X, (const T*)p.F1T + (int64_t)c0 * p.D1, p.M, t0, p.D1,
                           p.D1, gw, t);
    // ---- h = rn(s_c * H), s_c per column, padding columns zero -> this group's panels at byte offset c0 * 128 -----------
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = w + 4 * i;
      if (j < ntiles) {
        const int c = c0 + (j >> 1) * 32 + li;
        const float sc = c < r_acc ? 1.f : p.scale;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg)
          *(T*)(smem + cw_panel_off<T>((j & 1) * 32 + acc_row(reg, lane), c)) = from_f32<T>(c < r_tot ? sc * acc[i][reg] : 0.f);
      }
    }
    // (the next group's phase 1 writes the stage only, behind a barrier of its own)
  }
  __syncthreads();
  // ---- the live columns -> Hsave [M][64], as chain_wide_acc_kernel leaves them: data below r_live, zeros above, 1.0 in
  // column 63 when r_live < 64; 8 lanes write one whole 128-byte row
  if (p.Hsave) {
    const int t = threadIdx.x;
    T* H = (T*)p.Hsave;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int row = pass * 32 + (t >> 3), c0 = (t & 7) * 8;
      const int64_t gt = t0 + row;
      u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = c0 + 2 * q;   // r_acc and r_live are even: a pair is data or padding as a whole, and 4-byte aligned
        if (c < r_live) v[q] = *(const uint32_t*)(smem + cw_panel_off<T>(row, r_acc + c));
      }
      if (c0 == 56 && r_live < 64) v[3] = (v[3] & 0xffffu) | (DT<T>::one_bits << 16);
      if (gt < p.M) store_b128_nt(H + gt * 64 + c0, v);   // (carries the wait states a 16-byte store needs before v is rewritten)
    }
  }

  // ---- phase 2: Y = rn(h . [Fa2 ; Fl2] + bias) over all panels, 64 output columns at a time, one rounding ----------------
  cw_phase2_panels<T>(smem, stage, 4, &p.pan, (T*)p.Y, p.M, t0, p.D2, 0.f, p.nt_store != 0, threadIdx.x, (const T*)p.bias);
}

// The admitted set of SOW_FUSE_ACC_DEEP (include/sow_amd.h), a pure function of the shape and the compute dtype; disjoint
// from fused_acc_shape_ok by the total
bool deep_acc_shape_ok(int r_live, int r_acc, int d_in, int d_out, int dtype) {
  return (dtype == SOW_BF16 || dtype == SOW_F16) && r_live >= 2 && r_live <= 64 && r_live % 2 == 0 && r_acc >= 2 &&
         r_acc % 2 == 0 && r_acc <= DEEP_MAX_TOT && r_acc + r_live > 256 && r_acc + r_live <= DEEP_MAX_TOT && d_in > 0 &&
         d_out > 0 && d_in % 8 == 0 && d_out % 8 == 0;
}
size_t deep_acc_lds_bytes(int r_tot) { return (size_t)((r_tot + 63) / 64 * 64) * 128 + DEEP_STAGE; }

int launch_chain_deep_acc(const WideAccArgs& a, int dtype, hipStream_t stream) {
  if (!deep_acc_shape_ok(a.r_live, a.r_acc, a.D1, a.D2, dtype)) return SOW_ERR_UNSUPPORTED;
  if (!al16p(a.X) || !al16p(a.Y) || !al16p(a.bias) || !al16p(a.Hsave) || !a.pack || !al16p(a.pack) ||
      a.pack_bytes < chain_wide_pack_bytes(a.r_acc + a.r_live, a.D1, a.D2))
    return SOW_ERR_UNSUPPORTED;
  const size_t lds = deep_acc_lds_bytes(a.r_acc + a.r_live);
  if (lds > DEEP_MAX_LDS) return SOW_ERR_UNSUPPORTED;   // (cannot happen inside the admitted set: the plan's own guard)
  if (a.M <= 0) return SOW_OK;
  if (ceil_div(a.M, 64) > 0x7fffffff) return SOW_ERR_SHAPE;
  const WideAccPackParams pk = wide_acc_pack_params(a);
  DeepAccParams p{};
  p.pan.np = pk.r_pad / 64;
  if (p.pan.np > CW_MAXP) return SOW_ERR_UNSUPPORTED;   // (the table's own guard, as in launch_chain_shared_acc)
  for (int q = 0; q < p.pan.np; ++q) {
    p.pan.f2[q] = (const char*)pk.f2t + q * 128;
    p.pan.ld[q] = pk.r_pad;
  }
  p.X = a.X, p.Y = a.Y, p.F1T = pk.f1t, p.Hsave = a.Hsave, p.bias = a.bias;
  p.M = a.M, p.D1 = a.D1, p.D2 = a.D2, p.r_acc = a.r_acc, p.r_live = a.r_live, p.r_pad = pk.r_pad;
  p.scale = a.scale;
  p.nt_store = SOW_GEMM_NT(a.M) ? 1 : 0;
  const dim3 pgrid((unsigned)((pk.n + 255) / 256)), grid((unsigned)ceil_div(a.M, 64));
  if (dtype == SOW_BF16) {
    SOW_SET_MAX_LDS_ONCE((int)DEEP_MAX_LDS, chain_deep_acc_kernel<bf16_t>);
    hipLaunchKernelGGL(wide_acc_pack_kernel<bf16_t>, pgrid, dim3(256), 0, stream, pk);
    hipLaunchKernelGGL(chain_deep_acc_kernel<bf16_t>, grid, dim3(256), (unsigned)lds, stream, p);
  } else {
    SOW_SET_MAX_LDS_ONCE((int)DEEP_MAX_LDS, chain_deep_acc_kernel<f16_t>);
    hipLaunchKernelGGL(wide_acc_pack_kernel<f16_t>, pgrid, dim3(256), 0, stream, pk);
    hipLaunchKernelGGL(chain_deep_acc_kernel<f16_t>, grid, dim3(256), (unsigned)lds, stream, p);
  }
  SOW_CHECK_LAUNCH();
  return SOW_OK;
}

}  // namespace sow
