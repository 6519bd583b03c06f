// Shared-input data gradient of sibling layers that carry a low-rank accumulator (bf16 / f16): the fused chains of
// chain_wide_acc.hip, one per sibling, over ONE token block, their dX summed on chip (sow_backward_shared with SOW_FUSE_ACC,
// include/sow_amd.h).  For siblings i = 0 .. n - 1 (n <= 4) on one input of width D2 = d_in:
//
//   H_i  = dY_i . [R_i^T | B_i^T]                 [64 tokens x r_pad_i], fp32, r_pad_i = ceil64(r_acc_i + r_i), K = d_out_i
//   h_i  = [rn(H_i) | rn(scale_i H_i)]            accumulator columns | live columns, padding columns exact zeros; kept in
//                                                 LDS as r_pad_i / 64 panels; the live columns leave as dh_i [M, 64]
//   dX   = rn(beta dX + sum_i h_i . [Q_i^T ; A_i^T])   one fp32 accumulation over sibling 0's panels in ascending k, then
//                                                 sibling 1's, ...; ONE rounding, dX written once
//
// Phase 1 is cw_phase1 of the single fused pass with the same operands, so every h_i -- and the dh_i the weight-gradient
// kernels read -- has the bits chain_wide_acc_kernel leaves.  No atomics, a fixed order: a repeated call gives the same bits.
//
// The factors of all siblings are packed by ONE launch (shared_acc_pack_kernel) into each sibling's own pack region, in the
// image layout of launch_chain_wide_acc(bwd = 1): the data phase is two launches whatever n.
//
// Workgroup = 256 threads (4 waves), 64 tokens.  Dynamic LDS, sized from the set (sha_lds):
//   [ H panels: sum_i r_pad_i x 128 B ][ stage: the F1 image of a sibling (r_pad_i x 128 B) and its X image (8 KiB) in phase
//   1; in phase 2 g F2 panels of 8 KiB at a time (g = 3 or 4), then the epilogue scratch (18 KiB) ]
// q / k / v at r_pad = 128 each: 48 + 24 = 72 KiB, two workgroups per CU; three siblings of r_pad = 256: 96 + 40 = 136 KiB,
// one workgroup per CU.  A set is admitted when the plan fits into 160 KiB.
// The largest admitted set is r_pad = 256, 256, 256, 192: 120 + 40 = exactly 160 KiB, 15 panels (four of 256 plan 168 KiB).
#include <type_traits>

#include "chain_wide_tile.hpp"
#include "lds_dma.hpp"

namespace sow {

constexpr int SHA_MAXN = 4;
constexpr size_t SHA_MAX_LDS = 160 * 1024;

struct SharedAccPackTable {
  WideAccPackParams it[SHA_MAXN];
  int start[SHA_MAXN + 1];   // first block of item s; entries past the last item hold the grid size
};

template <typename T> __global__ __launch_bounds__(256) void shared_acc_pack_kernel(const SharedAccPackTable tb) {
  const int b = blockIdx.x;
  int s = 0;
#pragma unroll
  for (int k = 1; k < SHA_MAXN; ++k) s += b >= tb.start[k] ? 1 : 0;
  const WideAccPackParams& p = tb.it[s];
  const int64_t i = (int64_t)(b - tb.start[s]) * 256 + threadIdx.x;
  if (i < p.n) wide_acc_pack_elem<T>(p, i);
}

struct SharedAccSib {
  const void* X;     // dY_i [M][D1]
  const void* F1T;   // [r_pad][D1]
  void* Hsave;       // dh_i [M][64]
  int D1, r_acc, r_live, r_pad;
  float scale;
  int hoff;          // byte offset of this sibling's panels in the H region
};
struct SharedAccParams {
  SharedAccSib s[SHA_MAXN];
  CwPanels pan;      // the panels of all siblings in order, each with its slice of the sibling's F2T [D2][r_pad]
  void* Y;           // dX [M][D2]
  int64_t M;
  int D2, n, g;
  int stage_off, x_off;   // bytes: the stage after the H panels, the X image inside the stage
  float beta;
  int nt_store;
};
// every sibling has r_pad <= 256 (fused_acc_shape_ok): at most four panels each, so the table holds any set of SHA_MAXN
static_assert(CW_MAXP >= SHA_MAXN * (256 / 64), "the panel table must hold every sibling's panels");

// The parameter block is read where it lies, in the kernel-argument segment: the entry of sibling s and of panel q is then a
// scalar load at a uniform index, not a register copy of every entry.  This holds only while SharedAccParams is the kernel's
// FIRST explicit argument (explicit arguments start the segment, each laid out as the host lays it out): put no argument
// before it, and keep the struct plain data.
static_assert(std::is_trivially_copyable<SharedAccParams>::value && std::is_standard_layout<SharedAccParams>::value,
              "SharedAccParams is read from the kernel-argument segment as it is laid out on the host");
#define SHA_KARG __attribute__((address_space(4)))
template <typename T> __global__ __launch_bounds__(256, 2) void chain_shared_acc_kernel(const SharedAccParams) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const SharedAccParams SHA_KARG& p = *(const SharedAccParams SHA_KARG*)__builtin_amdgcn_kernarg_segment_ptr();
  char* stage = smem + p.stage_off;
  char* ximg = stage + p.x_off;

  const int64_t t0 = (int64_t)blockIdx.x * 64;

  for (int s = 0; s < p.n; ++s) {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));   // keeps the per-lane address arithmetic inside the iteration (as chain2_kernel does)
    const int lane = t & 63, w = t >> 6, li = lane & 31;
    const SharedAccSib SHA_KARG& S = p.s[s];
    char* hp = smem + S.hoff;
    const int r_pad = S.r_pad, ntiles = 2 * (r_pad / 32), r_acc = S.r_acc, r_live = S.r_live, r_tot = r_acc + r_live;
    // ---- phase 1: H_i = dY_i . [R_i^T | B_i^T] (chain_wide_tile.hpp), the F1 and X images in the stage -----------------
    f32x16 acc[4];
    cw_phase1_at<T, false>(acc, stage, ximg, (const T*)S.X, (const T*)S.F1T, p.M, t0, S.D1, S.D1, r_pad, t);
    // ---- h_i = rn(s_c * H_i), s_c per column, padding columns zero -> this sibling's panels ----------------------------
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = w + 4 * i;
      if (j < ntiles) {
        const int c = (j >> 1) * 32 + li;
        const float sc = c < r_acc ? 1.f : S.scale;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg)
          *(T*)(hp + cw_panel_off<T>((j & 1) * 32 + acc_row(reg, lane), c)) = from_f32<T>(c < r_tot ? sc * acc[i][reg] : 0.f);
      }
    }
    __syncthreads();
    // ---- the live columns -> dh_i [M][64], as chain_wide_acc_kernel leaves them: data below r_live, zeros above, 1.0 in
    // column 63 when r_live < 64; 8 lanes write one whole 128-byte row
    T* H = (T*)S.Hsave;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int row = pass * 32 + (t >> 3), c0 = (t & 7) * 8;
      const int64_t gt = t0 + row;
      u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = c0 + 2 * q;   // r_acc and r_live are even: a pair is data or padding as a whole, and 4-byte aligned
        if (c < r_live) v[q] = *(const uint32_t*)(hp + cw_panel_off<T>(row, r_acc + c));
      }
      if (c0 == 56 && r_live < 64) v[3] = (v[3] & 0xffffu) | (DT<T>::one_bits << 16);
      if (gt < p.M) store_b128_nt(H + gt * 64 + c0, v);
    }
    // (the next sibling's phase 1 writes the stage only, behind a barrier of its own)
  }

  // ---- phase 2: dX = rn(beta dX + sum_i h_i . [Q_i^T ; A_i^T]), 64 columns of d_in at a time, one rounding ----------------
  cw_phase2_panels<T>(smem, stage, p.g, &p.pan, (T*)p.Y, p.M, t0, p.D2, p.beta, p.nt_store != 0, threadIdx.x,
                      (const T*)nullptr);
}

// The LDS plan of a set (r_tot[i] = r_acc_i + r_i): bytes of the H panels, of the stage, and the F2 panels per group
struct ShaLds {
  size_t panels, stage;
  int x_off, g;
};
static ShaLds sha_lds(const int* r_tot, int n) {
  ShaLds l{};
  int rmax = 0;
  for (int i = 0; i < n; ++i) {
    const int r_pad = (r_tot[i] + 63) / 64 * 64;
    l.panels += (size_t)r_pad * 128;
    if (r_pad > rmax) rmax = r_pad;
  }
  l.x_off = rmax * 128;
  l.stage = (size_t)l.x_off + 8192;          // phase 1: the widest F1 image and the X image
  if (l.stage < 24576) l.stage = 24576;      // phase 2: the epilogue scratch (18 KiB) in whole panels
  l.g = l.stage / CW_PANEL < 4 ? (int)(l.stage / CW_PANEL) : 4;
  return l;
}
size_t shared_acc_lds_bytes(const int* r_tot, int n) {
  if (n < 1 || n > SHA_MAXN) return 0;
  const ShaLds l = sha_lds(r_tot, n);
  return l.panels + l.stage;
}
bool shared_acc_lds_ok(const int* r_tot, int n) {
  const size_t b = shared_acc_lds_bytes(r_tot, n);
  return b != 0 && b <= SHA_MAX_LDS;
}

int launch_chain_shared_acc(const WideAccArgs* sib, int n, void* dX, float beta, int dtype, hipStream_t stream) {
  if (n < 1 || n > SHA_MAXN || !dX || !al16p(dX)) return SOW_ERR_UNSUPPORTED;
  int r_tot[SHA_MAXN];
  for (int i = 0; i < n; ++i) {
    const WideAccArgs& a = sib[i];
    if (!a.bwd || a.M != sib[0].M || a.D2 != sib[0].D2 || !fused_acc_shape_ok(a.r_live, a.r_acc, a.D1, a.D2, dtype))
      return SOW_ERR_UNSUPPORTED;
    if (!a.X || !al16p(a.X) || !a.Hsave || !al16p(a.Hsave) || !a.pack || !al16p(a.pack) ||
        a.pack_bytes < chain_wide_pack_bytes(a.r_acc + a.r_live, a.D1, a.D2))
      return SOW_ERR_UNSUPPORTED;
    r_tot[i] = a.r_acc + a.r_live;
  }
  if (!shared_acc_lds_ok(r_tot, n)) return SOW_ERR_UNSUPPORTED;
  int panels = 0;
  for (int i = 0; i < n; ++i) panels += (r_tot[i] + 63) / 64;
  if (panels > CW_MAXP) return SOW_ERR_UNSUPPORTED;   // (cannot happen under the static_assert above: the table's own guard)
  const int64_t M = sib[0].M;
  if (M <= 0) return SOW_OK;
  if (ceil_div(M, 64) > 0x7fffffff) return SOW_ERR_SHAPE;
  const ShaLds l = sha_lds(r_tot, n);
  SharedAccPackTable tb{};
  SharedAccParams p{};
  int blocks = 0, hoff = 0, np = 0;
  for (int i = 0; i < n; ++i) {
    const WideAccArgs& a = sib[i];
    const WideAccPackParams pk = wide_acc_pack_params(a);
    tb.it[i] = pk;
    tb.start[i] = blocks;
    blocks += (int)((pk.n + 255) / 256);
    SharedAccSib& S = p.s[i];
    S.X = a.X, S.F1T = pk.f1t, S.Hsave = a.Hsave;
    S.D1 = a.D1, S.r_acc = a.r_acc, S.r_live = a.r_live, S.r_pad = pk.r_pad, S.scale = a.scale, S.hoff = hoff;
    hoff += pk.r_pad * 128;
    for (int pn = 0; pn < pk.r_pad / 64; ++pn, ++np) {
      p.pan.f2[np] = (const char*)pk.f2t + pn * 128;
      p.pan.ld[np] = pk.r_pad;
    }
  }
  for (int i = n; i <= SHA_MAXN; ++i) tb.start[i] = blocks;
  p.pan.np = np;
  p.Y = dX, p.M = M, p.D2 = sib[0].D2, p.n = n, p.g = l.g;
  p.stage_off = (int)l.panels, p.x_off = l.x_off, p.beta = beta;
  p.nt_store = SOW_GEMM_NT(M) ? 1 : 0;
  const unsigned lds = (unsigned)(l.panels + l.stage);
  const dim3 pgrid((unsigned)blocks), grid((unsigned)ceil_div(M, 64));
  if (dtype == SOW_BF16) {
    SOW_SET_MAX_LDS_ONCE((int)SHA_MAX_LDS, chain_shared_acc_kernel<bf16_t>);
    hipLaunchKernelGGL(shared_acc_pack_kernel<bf16_t>, pgrid, dim3(256), 0, stream, tb);
    hipLaunchKernelGGL(chain_shared_acc_kernel<bf16_t>, grid, dim3(256), lds, stream, p);
  } else {
    SOW_SET_MAX_LDS_ONCE((int)SHA_MAX_LDS, chain_shared_acc_kernel<f16_t>);
    hipLaunchKernelGGL(shared_acc_pack_kernel<f16_t>, pgrid, dim3(256), 0, stream, tb);
    hipLaunchKernelGGL(chain_shared_acc_kernel<f16_t>, grid, dim3(256), lds, stream, p);
  }
  SOW_CHECK_LAUNCH();
  return SOW_OK;
}

}  // namespace sow
