// extern "C" entry points of libsow_amd.so (declared in include/sow_amd.h).
// Host-side dispatch only: picks the fused low-rank chain / skinny-TN kernels for r <= 64 and composes
// the dense GEMM kernel for everything else.  No allocation, no synchronisation; the only process-wide state is the
// table of kernel-selection switches below (atomics, read from the environment once).
#include "kernels.hpp"
#include <cstring>
#include <vector>
#include <cstdio>
#include <cstdlib>

namespace sow {

// column sums of a [T, D] matrix (fallback path only: r_live > 64 with bias); TO = T, or float (SOW_PARAM_F32)
template <typename T, typename TO>
__global__ __launch_bounds__(256) void colsum_kernel(const T* M, int64_t ld, int64_t rows, int D, TO* out, float beta) {
  __shared__ float red[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), w = threadIdx.x >> 6;
  float s = 0.f;
  if (c < D)
    for (int64_t i = w; i < rows; i += 4) s += to_f32(M[i * ld + c]);
  red[w][threadIdx.x & 63] = s;
  __syncthreads();
  if (w == 0 && c < D) {
    float v = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    if (beta != 0.f) v += beta * to_f32(out[c]);
    out[c] = from_f32<TO>(v);
  }
}
static int launch_colsum(const void* dy, int64_t T, int d_out, void* dbias, float beta, int dtype, int out_dtype,
                         hipStream_t stream) {
  const dim3 grid((d_out + 63) / 64);
  if (out_dtype != dtype && out_dtype != SOW_F32) return SOW_ERR_DTYPE;
  const bool o32 = out_dtype == SOW_F32;
  if (dtype == SOW_F32)
    hipLaunchKernelGGL((colsum_kernel<float, float>), grid, dim3(256), 0, stream, (const float*)dy, (int64_t)d_out, T, d_out, (float*)dbias, beta);
  else if (dtype == SOW_BF16 && o32)
    hipLaunchKernelGGL((colsum_kernel<bf16_t, float>), grid, dim3(256), 0, stream, (const bf16_t*)dy, (int64_t)d_out, T, d_out, (float*)dbias, beta);
  else if (dtype == SOW_BF16)
    hipLaunchKernelGGL((colsum_kernel<bf16_t, bf16_t>), grid, dim3(256), 0, stream, (const bf16_t*)dy, (int64_t)d_out, T, d_out, (bf16_t*)dbias, beta);
  else if (dtype == SOW_F16 && o32)
    hipLaunchKernelGGL((colsum_kernel<f16_t, float>), grid, dim3(256), 0, stream, (const f16_t*)dy, (int64_t)d_out, T, d_out, (float*)dbias, beta);
  else if (dtype == SOW_F16)
    hipLaunchKernelGGL((colsum_kernel<f16_t, f16_t>), grid, dim3(256), 0, stream, (const f16_t*)dy, (int64_t)d_out, T, d_out, (f16_t*)dbias, beta);
  else
    return SOW_ERR_DTYPE;
  SOW_CHECK_LAUNCH();
  return SOW_OK;
}
}  // namespace sow

// ---- kernel-selection switches (common.hpp: enum Switch) ----------------------------------------------
namespace sow {
static const char* const kSwitchNames[SW_COUNT] = {"FORCE_CHAIN_V1", "NO_SHORT_SPLIT", "NO_FUSED_H", "FORCE_GEMM_V1", "TN_NARROW",
                                                   "NO_GEMM3S",      "GEMM3S",         "GEMM3",      "NO_GROUPED",     "NO_PERSIST",     "NO_NT_STORE",    "NT_LOAD",        "NO_PAIR_FLUSH",  "F32_EXACT",
                                                   "NO_PARK16",      "TN_NO_NT_LOAD",  "NO_TN_ROWS",     "GEMM4",          "NO_GEMM4H",      "NO_CHAIN3F",     "NO_TN_F32Q",     "NO_SPLITK",
                                                   "NO_WIDE_CHAIN",  "NO_SHARED_X",    "NO_RAGGED",      "NO_RAGGED_GEMM", "NO_BLOCKED_QR",
                                                   "NO_SKINNY",      "NO_FUSED_ACC",   "NO_DEEP_ACC",    "NO_F16_TN",
                                                   "NO_ROW_ALIGN",   "NO_X_PAIR",      "NO_H_ROWS"};
static std::atomic<int> g_switch[SW_COUNT];
static std::once_flag g_switch_once;
static void switches_from_env() {
  for (int i = 0; i < SW_COUNT; ++i) {
    char name[64];
    snprintf(name, sizeof name, "SOW_AMD_%s", kSwitchNames[i]);
    const char* v = getenv(name);
    // tri-state switches take "0" / "1"; for the boolean ones any value (even empty) means on, as before
    const bool tri = i == SW_GEMM3S || i == SW_GEMM3 || i == SW_GEMM4;
    // NO_ROW_ALIGN keeps its value (1 = both sides off, 2 / 3 = one side)
    const int on = i == SW_NO_ROW_ALIGN && v && v[0] >= '1' && v[0] <= '3' ? v[0] - '0' : 1;
    g_switch[i].store(!v ? -1 : (tri ? (v[0] != '0') : on), std::memory_order_relaxed);
  }
}
int sw(int which) {
  std::call_once(g_switch_once, switches_from_env);
  return g_switch[which].load(std::memory_order_relaxed);
}
}  // namespace sow

using namespace sow;

static inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }
static inline size_t esize(int dtype) { return dtype == SOW_F32 ? 4 : 2; }
static inline bool ok_dtype(int d) { return d == SOW_F32 || d == SOW_BF16 || d == SOW_F16; }
// The dtype argument of an entry point, decoded once.  SOW_FUSE_ACC and SOW_FUSE_ACC_DEEP are permissions and are ignored
// together with SOW_PARAM_F32; SOW_ACC_NATIVE means something next to SOW_PARAM_F32 only.
// The layer entry points, their plans and descriptors take what layer_ok() admits; sow_*_shared refuses SOW_PARAM_F32 as
// unsupported after its own checks.  The entry points outside the layer surface (GEMM, QR, accumulate, optimizer, copies)
// only strip the permission with nofuse() and refuse or reject SOW_PARAM_F32 themselves, each with its own code.
struct Dtype {
  int cd;           // compute dtype: the argument without its flag bits (not validated)
  bool param_f32;   // SOW_PARAM_F32
  bool fuse;        // SOW_FUSE_ACC, without SOW_PARAM_F32
  bool deep;        // SOW_FUSE_ACC_DEEP, without SOW_PARAM_F32
  bool native;      // SOW_ACC_NATIVE next to SOW_PARAM_F32: the accumulator is of the compute dtype and is not packed
  bool native_bit;  // SOW_ACC_NATIVE as passed (ignored without SOW_PARAM_F32; refused where SOW_PARAM_F32 is refused)
  // the permission bits a layer call carries on (SOW_FUSE_ACC | SOW_FUSE_ACC_DEEP, or 0)
  int perm() const { return (fuse ? SOW_FUSE_ACC : 0) | (deep ? SOW_FUSE_ACC_DEEP : 0); }
  bool layer_ok() const { return ok_dtype(cd) && !((param_f32 || native_bit) && cd == SOW_F32); }   // fp32 compute takes neither flag
};
static inline Dtype decode_dtype(int d) {
  Dtype f;
  f.cd = d & ~(SOW_FUSE_ACC | SOW_FUSE_ACC_DEEP | SOW_PARAM_F32 | SOW_ACC_NATIVE);
  f.param_f32 = (d & SOW_PARAM_F32) != 0;
  f.native_bit = (d & SOW_ACC_NATIVE) != 0;
  f.native = f.native_bit && f.param_f32;
  f.fuse = (d & SOW_FUSE_ACC) != 0 && !f.param_f32;
  f.deep = (d & SOW_FUSE_ACC_DEEP) != 0 && !f.param_f32;
  return f;
}
static inline bool flagged(int d) { return (d & (SOW_PARAM_F32 | SOW_ACC_NATIVE)) != 0; }
static inline int nofuse(int d) { return d & ~(SOW_FUSE_ACC | SOW_FUSE_ACC_DEEP); }

// ---- short inputs ---------------------------------------------------------------------------------
// T / 64 workgroups cannot fill 256 CUs: below SHORT_NTB token blocks the streaming chain is launched as
// phase 1 split over K (fp32 partials + h_reduce) and phase 2 split over the output columns (kernels.hpp).
constexpr int SHORT_NTB = 128;
static inline int short_want(int ntb) { return ntb > 0 ? (256 + ntb - 1) / ntb : 1; }
static size_t short_hp_bytes(int64_t T, int d_in, int d_out, int r_live, int dtype) {
  const int ntb = ceil_div(T, 64);
  if (r_live > 64 || ntb <= 0 || ntb > SHORT_NTB) return 0;
  const int dmax = d_in > d_out ? d_in : d_out;
  int ks = short_want(ntb);
  const int nst = (dmax + 63) / 64;
  if (ks > nst) ks = nst;
  return al256((size_t)ks * (size_t)T * 64 * sizeof(float));
}
// the live-factor chain of one direction (Hsave required); returns SOW_ERR_UNSUPPORTED when the split does not apply
static int launch_chain_short(const ChainParams& p, int dtype, bool bwd, float* hpartial, hipStream_t stream) {
  const int ntb = ceil_div(p.M, 64);
  const bool f32 = dtype == SOW_F32;   // else bf16 / f16: chain2 (launch_chain2 dispatches on the dtype)
  if (!hpartial || !p.Hsave || ntb > SHORT_NTB || !(f32 ? chain2f_supported(p, dtype) : chain2_supported(p, dtype)) ||
      sw_on(SW_FORCE_CHAIN_V1) || sw_on(SW_NO_SHORT_SPLIT))
    return SOW_ERR_UNSUPPORTED;
  const int want = short_want(ntb);
  const int nst = (p.D1 + 63) / 64, nsl = (p.D2 + 63) / 64;
  if (nst + nsl < 24) return SOW_ERR_UNSUPPORTED;   // tiny layers: three launches cost more than the idle CUs (26 vs 19 us at 64 x 256 x 256)
  int rc;
  // phase 1: H = scale * X . F1
  int ks = want < nst ? want : nst;
  if (ks > 1) {
    ChainParams a = p;
    a.ntb = ntb, a.st_per = ceil_div(nst, ks), a.sl_per = 0, a.Hpartial = hpartial, a.Hload = nullptr;
    ks = ceil_div(nst, a.st_per);
    rc = f32 ? launch_chain2f(a, bwd, stream) : launch_chain2(a, bwd, dtype, stream);
    if (rc) return rc == SOW_ERR_ALIGN ? SOW_ERR_UNSUPPORTED : rc;
    rc = launch_h_reduce(hpartial, ks, p.Hsave, p.M, p.rb, p.scale, dtype, stream);
    if (rc) return rc;
  } else {
    ChainParams a = p;
    a.Y = nullptr, a.D2 = 0, a.bias = nullptr;   // H-only mode
    rc = f32 ? launch_chain2f(a, bwd, stream) : launch_chain2(a, bwd, dtype, stream);
    if (rc) return rc == SOW_ERR_ALIGN ? SOW_ERR_UNSUPPORTED : rc;
  }
  if (nsl == 0) return SOW_OK;
  // phase 2: Y = beta * Y + H . F2 + bias
  ChainParams b = p;
  const int kn = want < nsl ? want : nsl;
  b.ntb = ntb, b.st_per = 0, b.sl_per = ceil_div(nsl, kn), b.Hpartial = nullptr, b.Hload = p.Hsave, b.Hsave = nullptr;
  return f32 ? launch_chain2f(b, bwd, stream) : launch_chain2(b, bwd, dtype, stream);
}

// ---- dense products with a row-major A (trans_a = 0): which kernel writes C -----------------------------------------
// The one place where the kernel of  C = alpha (A . op(B) + A2 . op(B2)) + beta C + bias  is chosen.  pick_gemm reads the
// operands, the split-K scratch and the switches and launches nothing; launch_picked launches what it said.
// t256 / t128: output tiles of 256 x 256 / 128 x 128.  `work`: gemm4's workgroups, t256 x its K-splits with this scratch.
//   * gemm4 (anti-phase wave groups, 64-wide K-tiles) is 15-30 % faster than the older main loops wherever its tiles fill at
//     least half of the chip (work >= 120; profiles/r03_gemm4_vs_round2_vs_hipblaslt.txt: 4096^3 1.38 vs 0.97-1.03 PF, 32768 x
//     512 -> 1376 58 vs 72 us).  With scratch from the caller, short products (<= 128 tiles, long K) reach that split over K:
//     M = 1024 x N = 4096 as 64 tiles x 4 splits instead of gemm3s's 256 small tiles.  GEMM4 = 1 forces it on every shape it
//     supports, 0 forbids it.
//   * bf16 below that: with fewer than 160 big tiles the 128 x 128 tiles of gemm3s fill more CUs; from K ~ 2048 on the
//     one-wave-per-SIMD gemm3 is 7-19 % ahead of gemm2 (4096^3: 1.05 vs 0.90-0.96 PF), at K <= 1376 they are level or gemm2 is
//     ahead.  GEMM3S and GEMM3 = 1 / 0 force or forbid either.
//   * bf16 products too small for gemm3s (t128 < 96, or K < 512, or NO_GEMM3S) and every other dtype: the generic kernel.
// Asymmetries, kept as they were measured and tested:
//   * the bf16 gate stands before gemm4 and f16 has none: 120-159 big tiles with K < 512 are generic in bf16, gemm4 in f16;
//   * NO_GEMM3S acts only in the gate (a product that passes it may still take gemm3s); GEMM3S = 0 acts only after it;
//   * t256 >= 160 with 32 <= K < 64: gemm4 needs K >= 64, so bf16 takes gemm2_kernel by default;
//   * GEMM4 = 1 with K < 64 (gemm4_supported fails) falls through to the others.
enum GemmKernel { GEMM_GENERIC, GEMM_2, GEMM_3, GEMM_3S, GEMM_4 };
static GemmKernel pick_gemm(const ExtGemm& g, int dtype, const void* ws, size_t ws_bytes) {
  if (dtype != SOW_BF16 && dtype != SOW_F16) return GEMM_GENERIC;
  const int64_t t256 = (int64_t)ceil_div(g.M, 256) * ceil_div(g.N, 256);
  const int g4 = sw(SW_GEMM4);
  auto half_chip = [&] { return t256 * gemm4_splits(g.M, g.N, g.K, g.A2 != nullptr, ws, ws_bytes) >= 120; };
  if (dtype == SOW_F16) {
    // f16 has gemm4 (and its split-K form) only, and no caller with a K-extension
    const bool take = !g.A2 && !sw_on(SW_FORCE_GEMM_V1) && (g4 > 0 || (g4 < 0 && half_chip())) && gemm4_supported(g, dtype);
    return take ? GEMM_4 : GEMM_GENERIC;
  }
  // the bf16 gate
  if (!ext_gemm_operands_ok(g) || g.N < 64 || g.K < 32) return GEMM_GENERIC;
  const int64_t t128 = (int64_t)ceil_div(g.M, 128) * ceil_div(g.N, 128);
  if (t256 < 160 && (t128 < 96 || g.K < 512 || sw_on(SW_NO_GEMM3S))) return GEMM_GENERIC;
  if (sw_on(SW_FORCE_GEMM_V1)) return GEMM_GENERIC;   // A/B switch, as SOW_AMD_FORCE_CHAIN_V1
  if ((g4 > 0 || (g4 < 0 && half_chip() && g.K >= 64)) && gemm4_supported(g, SOW_BF16)) return GEMM_4;
  const int gs = sw(SW_GEMM3S);
  if (gs >= 0 ? gs != 0 : t256 < 160) return GEMM_3S;
  const int g3 = sw(SW_GEMM3);
  if (g3 >= 0 ? g3 != 0 : g.K >= 2048) return GEMM_3;
  return GEMM_2;
}
// dtype: of the call pick_gemm saw (gemm2 / gemm3 / gemm3s are picked for SOW_BF16 only); the generic kernel has no
// K-extension, so a product with one that no streaming kernel takes is refused (dense_ext_term asks before it launches)
static int launch_picked(GemmKernel k, const ExtGemm& g, int dtype, void* ws, size_t ws_bytes, hipStream_t stream) {
  switch (k) {
    case GEMM_4: return launch_gemm4(g, dtype, ws, ws_bytes, stream);
    case GEMM_3S: return launch_gemm3s(g, stream);
    case GEMM_3: return launch_gemm3(g, stream);
    case GEMM_2: return launch_gemm2(g, stream);
    default: break;
  }
  if (g.A2) return SOW_ERR_UNSUPPORTED;
  return launch_gemm(g.A, g.lda, false, g.B, g.ldb, g.nt, g.C, g.ldc, g.bias, g.M, g.N, g.K, g.alpha, g.beta, dtype, stream);
}
// the plain product C = alpha A . op(B) + beta C + bias on the kernel pick_gemm chooses
static int gemm_auto(const void* A, int64_t lda, const void* B, int64_t ldb, bool transB, void* C, int64_t ldc, const void* bias,
                     int64_t M, int N, int K, float alpha, float beta, int dtype, hipStream_t stream, void* ws = nullptr,
                     size_t ws_bytes = 0) {
  const ExtGemm g{A, B, nullptr, nullptr, C, bias, M, lda, ldb, 0, 0, ldc, N, K, 0, transB, alpha, beta};
  return launch_picked(pick_gemm(g, dtype, ws, ws_bytes), g, dtype, ws, ws_bytes, stream);
}

extern "C" {

int sow_version(void) { return 125; }

int sow_set_switch(const char* name, int value) {
  if (!name) return SOW_ERR_NULL;
  (void)sw(0);   // make sure the environment has been read first
  for (int i = 0; i < SW_COUNT; ++i)
    if (!strcmp(name, kSwitchNames[i])) {
      g_switch[i].store(value < 0 ? -1 : (i == SW_NO_ROW_ALIGN && value <= 3 ? value : (value != 0)), std::memory_order_relaxed);
      return SOW_OK;
    }
  return SOW_ERR_UNSUPPORTED;
}

#ifdef SOW_STAMPS
// debug builds only (not declared in include/sow_amd.h): device buffer for the in-kernel timeline of chain2_kernel
int sow_debug_set_stamps(void* buf) {
  g_chain2_stamps = buf;
  return SOW_OK;
}
#endif

int sow_get_switch(const char* name) {
  if (!name) return SOW_ERR_NULL;
  for (int i = 0; i < SW_COUNT; ++i)
    if (!strcmp(name, kSwitchNames[i])) return sw(i);
  return SOW_ERR_UNSUPPORTED;
}

const char* sow_error_string(int code) {
  switch (code) {
    case SOW_OK: return "ok";
    case SOW_ERR_NULL: return "null pointer argument";
    case SOW_ERR_SHAPE: return "invalid shape argument";
    case SOW_ERR_DTYPE: return "unsupported dtype";
    case SOW_ERR_ALIGN: return "misaligned pointer";
    case SOW_ERR_WORKSPACE: return "workspace too small";
    case SOW_ERR_UNSUPPORTED: return "unsupported configuration";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown error";
  }
}

size_t sow_h_save_elems(int64_t T, int r_live) { return (size_t)T * (size_t)(r_live <= 64 ? 64 : r_live); }

// A layer of ragged widths (include/sow_amd.h): bf16 / f16 compute dtype, even r_live in (64, 256], d_in or d_out not a
// multiple of 8, no accumulator, a dense one, or a low-rank one of even r_acc in [2, 256].  A pure function of the shape:
// the workspace plan follows it whatever the NO_RAGGED / NO_RAGGED_GEMM switches say.
static bool rag_layer(int r_live, int r_acc, int acc_kind, int d_in, int d_out, int dtype) {
  return r_live > 64 && ragged_shape_ok(r_live, d_in, d_out, dtype) &&
         (acc_kind == SOW_ACC_NONE || acc_kind == SOW_ACC_DENSE ||
          (acc_kind == SOW_ACC_LOWRANK && ragged_shape_ok(r_acc, d_in, d_out, dtype)));
}

// The dense-accumulator product of an admitted ragged layer (C = A . op(B), alpha = 1, beta = 0): gemm_rag, W_acc read in
// place; gemm_auto (the generic kernel at these widths) under NO_RAGGED_GEMM or where gemm_rag does not take the operands.
static int rag_dense_product(const void* A, int64_t lda, const void* B, int64_t ldb, bool transB, void* C, int64_t ldc, int64_t M,
                             int N, int K, int dtype, hipStream_t stream) {
  if (!sw_on(SW_NO_RAGGED_GEMM) && gemm_rag_supported(A, lda, B, ldb, transB, C, ldc, M, N, K, dtype))
    return launch_gemm_rag(A, lda, B, ldb, transB, C, ldc, M, N, K, dtype, stream);
  return gemm_auto(A, lda, B, ldb, transB, C, ldc, nullptr, M, N, K, 1.f, 0.f, dtype, stream);
}

// workspace carve (identical in the query and in the calls)
struct WsPlan {
  size_t off_dh, off_t, off_apad, off_hp, off_p0, off_p1, off_planes, planes_bytes, off_sk, sk_bytes, off_wide, wide_bytes,
      off_pw, pw_bytes, total;
  bool fused;   // the plan holds the pack region of the fused accumulator pass (SOW_FUSE_ACC on an admitted shape)
  bool deep;    // ... of the fused pass past 256 columns (SOW_FUSE_ACC_DEEP on an admitted shape)
  int ns, slab_len;
  int ns_cap;   // slabs the partial regions can hold (group-planned slab counts may exceed the single-layer choice)
};
constexpr int64_t C3F_MIN_T = 8192;   // chain3f_supported's threshold
// perm: the caller's permission bits (SOW_FUSE_ACC, SOW_FUSE_ACC_DEEP).  On a shape a bit admits (the two sets are disjoint
// by r_acc + r_live) the wide region also holds the factors of the fused pass (r_acc + r_live columns); such a layer has
// r_live <= 64, so the region is the plan's last and every other offset is the unflagged plan's -- the [T x r_acc] scratch of
// gemm_pair included: a flagged workspace serves the unflagged kernels as it is.  A pure function of its arguments.
static WsPlan plan_ws(int64_t T, int d_in, int d_out, int r_live, int r_acc, int acc_kind, int dtype, int perm = 0) {
  WsPlan w{};
  const size_t es = esize(dtype);
  size_t off = 0;
  w.off_dh = off;
  off += al256((size_t)T * (size_t)(r_live <= 64 ? 64 : r_live) * es);
  w.off_t = off;
  if (acc_kind == SOW_ACC_LOWRANK && r_acc > 64) off += al256((size_t)T * r_acc * es);
  w.off_apad = off;   // A zero-padded to [d_in, 64]: the k-contiguous K-extension operand of the dense backward
  if (acc_kind == SOW_ACC_DENSE && r_live <= 64) off += al256((size_t)d_in * 64 * es);
  w.off_hp = off;     // fp32 partial H of the short-T split: splits * T * 64 floats, splits <= 256 / ceil(T / 64)
  off += short_hp_bytes(T, d_in, d_out, r_live, dtype);
  if (r_live <= 64) {
    w.ns = tn_pick_slabs(T, d_in, d_out, dtype, &w.slab_len);
    w.ns_cap = w.ns;
    // both 16-bit dtypes (a pure function of shape and dtype: NO_F16_TN does not shrink the f16 workspace)
    if ((dtype == SOW_BF16 || dtype == SOW_F16) && T >= 1024) {
      const int by_len = (int)(T / 512 < TNR_MAX_SLABS ? T / 512 : TNR_MAX_SLABS);
      if (by_len > w.ns_cap) w.ns_cap = by_len;
    }
    w.off_p0 = off;
    off += al256(tn_partial_bytes(w.ns_cap, d_in));
    w.off_p1 = off;
    off += al256(tn_partial_bytes(w.ns_cap, d_out));
  }
  // fp32 streaming chain (chain3f.hip): the factors of a launch pre-split into bf16 planes, 24 KiB per 64-wide chunk of
  // d_in and of d_out (either direction; a low-rank accumulator's chain reuses the region: same stream, launch after launch)
  w.off_planes = off;
  w.planes_bytes = 0;
  if (dtype == SOW_F32 && T >= C3F_MIN_T && (r_live <= 64 || (acc_kind == SOW_ACC_LOWRANK && r_acc <= 64))) {
    w.planes_bytes = chain3f_plane_bytes(d_in, d_out);
    off += al256(w.planes_bytes);
  }
  // split-K scratch of the dense-accumulator products of short inputs (gemm4.hip): forward [T, d_out] over K = d_in (+ the
  // rank extension), backward [T, d_in] over K = d_out
  w.off_sk = off;
  w.sk_bytes = 0;
  if (dtype == SOW_BF16 && acc_kind == SOW_ACC_DENSE) {
    const size_t f = gemm4_splitk_bytes(T, d_out, d_in, true), b = gemm4_splitk_bytes(T, d_in, d_out, true);
    w.sk_bytes = f > b ? f : b;
    off += al256(w.sk_bytes);
  }
  // fused wide-rank chain (chain_wide.hip): the packed factors of one launch -- the live factors or those of a wide low-rank
  // accumulator (same stream, launch after launch: they share the region)
  w.off_wide = off;
  w.wide_bytes = 0;
  {
    int rw = chain_wide_shape_ok(r_live, d_in, d_out, dtype) ? r_live : 0;
    if (acc_kind == SOW_ACC_LOWRANK && chain_wide_shape_ok(r_acc, d_in, d_out, dtype) && r_acc > rw) rw = r_acc;
    // ragged layer: the factors of its live term or of its low-rank accumulator, whichever is wider
    if (rag_layer(r_live, r_acc, acc_kind, d_in, d_out, dtype)) rw = acc_kind == SOW_ACC_LOWRANK && r_acc > r_live ? r_acc : r_live;
    if (rw) w.wide_bytes = chain_wide_pack_bytes(rw, d_in, d_out);
    w.fused = (perm & SOW_FUSE_ACC) && acc_kind == SOW_ACC_LOWRANK && fused_acc_shape_ok(r_live, r_acc, d_in, d_out, dtype);
    w.deep = (perm & SOW_FUSE_ACC_DEEP) && acc_kind == SOW_ACC_LOWRANK && deep_acc_shape_ok(r_live, r_acc, d_in, d_out, dtype);
    if (w.fused || w.deep) {
      const size_t fb = chain_wide_pack_bytes(r_acc + r_live, d_in, d_out);
      if (fb > w.wide_bytes) w.wide_bytes = fb;
    }
    off += al256(w.wide_bytes);
  }
  // token-slab partials of the wide weight-gradient kernel (skinny_tn_wide.hip), whatever NO_WIDE_CHAIN / NO_RAGGED say;
  // pw_bytes != 0 is the shape half of pick_tn_wide_rank
  w.off_pw = off;
  w.pw_bytes = 0;
  if (tnw_shape_ok(r_live, d_in, d_out, dtype) || rag_layer(r_live, r_acc, acc_kind, d_in, d_out, dtype)) {
    w.pw_bytes = tnw_partial_bytes(T, d_in, d_out, r_live);
    off += al256(w.pw_bytes);
  }
  w.total = off;
  return w;
}

static char* ws_base(void* workspace) {
  uintptr_t a = reinterpret_cast<uintptr_t>(workspace);
  return reinterpret_cast<char*>((a + 255) & ~(uintptr_t)255);
}
// hands the factor-plane scratch of the workspace to a chain launch (fp32, long T: chain3f.hip); without it the launch
// takes chain2f
static void set_planes(ChainParams& p, char* ws, const WsPlan& w, size_t workspace_bytes) {
  if (ws && w.planes_bytes && workspace_bytes >= w.total) p.planes = ws + w.off_planes, p.planes_bytes = w.planes_bytes;
}

// ---- one layer ------------------------------------------------------------------------------------------------------
// Every layer entry point works on a sow_layer_args: the single-layer entry points build one from their arguments, the
// grouped and shared ones pass their elements through.
static sow_layer_args single_layer(const void* x, const void* A, const void* B, const void* acc_down, const void* acc_up,
                                   const void* bias, void* y, void* h_save, const void* dy, void* dx, void* dA, void* dB,
                                   void* dbias, int64_t T, int d_in, int d_out, int r_live, int r_acc, int acc_kind, float scale,
                                   float grad_beta, void* workspace, size_t workspace_bytes) {
  sow_layer_args L{};
  L.x = x, L.A = A, L.B = B, L.acc_down = acc_down, L.acc_up = acc_up, L.bias = bias, L.y = y, L.h_save = h_save;
  L.dy = dy, L.dx = dx, L.dA = dA, L.dB = dB, L.dbias = dbias;
  L.T = T, L.d_in = d_in, L.d_out = d_out, L.r_live = r_live, L.r_acc = r_acc, L.acc_kind = acc_kind;
  L.scale = scale, L.grad_beta = grad_beta, L.workspace = workspace, L.workspace_bytes = workspace_bytes;
  return L;
}
// r_acc counts only for a low-rank accumulator
static inline int acc_rank(const sow_layer_args& L) { return L.acc_kind == SOW_ACC_LOWRANK ? L.r_acc : 0; }
// the accumulator fields a layer's kind does not use, cleared (before the parameters are packed: pack_layer)
static void normalise_acc(sow_layer_args& L) {
  if (L.acc_kind != SOW_ACC_LOWRANK) L.r_acc = 0, L.acc_up = nullptr;
  if (L.acc_kind == SOW_ACC_NONE) L.acc_down = nullptr;
}
// A quantised accumulator (codes and scales: acc_is_codes) is read by sow_forward_skinny only: every other layer entry point asks
// here first, before any other check, launch or dereference
static inline bool any_codes_acc(const sow_layer_args* layers, int n) {
  if (layers)
    for (int i = 0; i < n; ++i)
      if (acc_is_codes(layers[i].acc_kind)) return true;
  return false;
}
static inline WsPlan plan_of(const sow_layer_args& L, int cd, int perm = 0) {
  return plan_ws(L.T, L.d_in, L.d_out, L.r_live, acc_rank(L), L.acc_kind, cd, perm);
}
// The argument checks of a layer, in the one order every entry point reports them: shape, then (T > 0 only) NULL operands,
// then a missing accumulator (NULL), then, with `lowrank`, the second factor and rank of a low-rank accumulator (SHAPE).
// T = 0 is valid whatever the pointers are.  What differs between the entry points is what they test BEFORE this and where
// they call it; none of that may move across a launch:
//   forward_impl, and sow_forward under SOW_PARAM_F32 (before the pack launch): dtype first.
//   backward_impl: phases (SHAPE), then dtype, then this; at T = 0 it wants dA and dB (NULL).
//   sow_backward_ex under SOW_PARAM_F32: dtype first, then -- DATA phase with T > 0 only, before the pack launch -- this, then
//     backward_impl's sequence again.
//   groups: dtype (backward: phases first when unflagged), n, layers; then this WITHOUT `lowrank`, for every layer up front
//     (backward, plans, shared) or layer by layer between the launches (forward).  A low-rank accumulator without acc_up is
//     refused by the per-layer fall-through (forward_impl / backward_impl), after the layers before it have been enqueued.
//   pack_group (groups under SOW_PARAM_F32): this WITH `lowrank`, for every layer before the one pack launch.
//   sow_forward_skinny has checks of its own, stricter and all before any launch.
static int check_layer(const sow_layer_args& L, bool bwd, bool lowrank) {
  if (L.T < 0 || L.d_in <= 0 || L.d_out <= 0 || L.r_live <= 0) return SOW_ERR_SHAPE;
  if (L.T == 0) return SOW_OK;
  if (!L.x || !L.A || !L.B) return SOW_ERR_NULL;
  if (!bwd && !L.y) return SOW_ERR_NULL;
  if (bwd && (!L.dy || !L.h_save || !L.dx || !L.dA || !L.dB || !L.workspace)) return SOW_ERR_NULL;
  if (L.acc_kind != SOW_ACC_NONE && !L.acc_down) return SOW_ERR_NULL;
  if (lowrank && L.acc_kind == SOW_ACC_LOWRANK && (!L.acc_up || L.r_acc <= 0)) return SOW_ERR_SHAPE;
  return SOW_OK;
}

// ---- fp32 parameters (SOW_PARAM_F32) ----------------------------------------------------------------------
// The fp32 A, B, bias and accumulator of a call are rounded once to the compute dtype into a region of the layer's workspace
// past the compute-dtype plan (pack_params_kernel, misc.hip); the bf16 / f16 kernels then read the packed copies, in the
// layouts they read from the caller.  Packed again at every call: the factors change at every optimizer step.
static inline size_t pack_elems_bytes(int64_t n) { return al256((size_t)n * 2); }
// native (SOW_ACC_NATIVE): the accumulator is of the compute dtype already; the kernels read it where it lies
static size_t pack_bytes(int d_in, int d_out, int r_live, int r_acc, int acc_kind, bool native) {
  size_t b = pack_elems_bytes((int64_t)d_in * r_live) + pack_elems_bytes((int64_t)r_live * d_out) + pack_elems_bytes(d_out);
  if (native) return b;
  if (acc_kind == SOW_ACC_DENSE) b += pack_elems_bytes((int64_t)d_in * d_out);
  if (acc_kind == SOW_ACC_LOWRANK) b += pack_elems_bytes((int64_t)d_in * r_acc) + pack_elems_bytes((int64_t)r_acc * d_out);
  return b;
}
// Appends the pack items of layer L (T > 0, checked and normalised) to `items` and points L's parameter operands at the
// packed copies.  The packed copies go past the compute-dtype plan (where they never touch what a backward phase leaves in
// the workspace), except for a forward (fwd) whose kernels need no scratch (sow_forward_workspace_bytes = 0 for the compute
// dtype) given a workspace sized by the flagged forward query only: there they start the workspace.  Such a forward then runs
// without workspace, exactly as the unflagged call.
static int pack_layer(sow_layer_args& L, int cd, bool fwd, bool native, std::vector<PackItem>& items) {
  const int r_acc = acc_rank(L);
  const WsPlan w = plan_of(L, cd);
  const size_t pack = pack_bytes(L.d_in, L.d_out, L.r_live, r_acc, L.acc_kind, native);
  const bool no_scratch = fwd && sow_forward_workspace_bytes(L.T, L.d_in, L.d_out, L.r_live, r_acc, L.acc_kind, cd) == 0;
  const size_t off = (no_scratch && L.workspace_bytes < w.total + pack + 255) ? 0 : w.total;
  if (!L.workspace) return SOW_ERR_NULL;
  if (L.workspace_bytes < off + pack + 255) return SOW_ERR_WORKSPACE;
  char* dst = ws_base(L.workspace) + off;
  if (no_scratch) L.workspace = nullptr, L.workspace_bytes = 0;
  auto put = [&](const void*& src, int64_t n) {
    if (!src) return;
    items.push_back(PackItem{(const float*)src, dst, n});
    src = dst;
    dst += pack_elems_bytes(n);
  };
  put(L.A, (int64_t)L.d_in * L.r_live);
  put(L.B, (int64_t)L.r_live * L.d_out);
  put(L.bias, L.d_out);
  if (native) return SOW_OK;
  if (L.acc_kind == SOW_ACC_DENSE) put(L.acc_down, (int64_t)L.d_in * L.d_out);
  if (L.acc_kind == SOW_ACC_LOWRANK) {
    put(L.acc_down, (int64_t)L.d_in * r_acc);
    put(L.acc_up, (int64_t)r_acc * L.d_out);
  }
  return SOW_OK;
}
// one layer of a single-layer call: checked as the unflagged call checks it, packed by a launch of its own
static int pack_single(sow_layer_args& L, int cd, bool fwd, bool native, hipStream_t stream) {
  int rc = check_layer(L, !fwd, true);
  if (rc) return rc;
  normalise_acc(L);
  std::vector<PackItem> items;
  if ((rc = pack_layer(L, cd, fwd, native, items))) return rc;
  return launch_pack_params(items.data(), (int)items.size(), cd, stream);
}

// ---- one direction of a layer ---------------------------------------------------------------------------------------
// What the chain kernels compute is  H = X . F1,  Y = beta Y + H . F2  for a pair of factors `down` [d_in][r] (row pitch r)
// and `up` [r][d_out] (row pitch d_out): the live pair (A, B) or a low-rank accumulator (acc_down, acc_up).
//   forward:        X = x,  Y = y,  D1 = d_in,  D2 = d_out, F1 = down, F2 = up,   H = h_save, bias
//   data gradient:  X = dY, Y = dX, D1 = d_out, D2 = d_in,  F1 = up,   F2 = down, H = dh (workspace), no bias
// A dense accumulator W [d_in][d_out] is read as it lies by the forward and transposed by the data gradient.
// This is the only place that knows the mapping; the launches below are written once for both directions.
struct Factors {
  const void *F1, *F2;
  int64_t ld1, ld2;
  int r;
};
struct DirView {
  bool bwd;
  const void* X;
  void* Y;
  void* H;
  const void* bias;
  int64_t M;
  int D1, D2;
  Factors live, acc;
  const void* W;
  int64_t ldw;
  float scale;   // of the live term
};
static Factors factor_pair(const void* down, const void* up, int r, int d_out, bool bwd) {
  return bwd ? Factors{up, down, d_out, r, r} : Factors{down, up, r, d_out, r};
}
static DirView dir_view(const sow_layer_args& L, bool bwd, void* dh) {
  DirView v{};
  v.bwd = bwd, v.M = L.T, v.scale = L.scale;
  v.X = bwd ? L.dy : L.x, v.Y = bwd ? L.dx : L.y, v.H = bwd ? dh : L.h_save, v.bias = bwd ? nullptr : L.bias;
  v.D1 = bwd ? L.d_out : L.d_in, v.D2 = bwd ? L.d_in : L.d_out;
  v.live = factor_pair(L.A, L.B, L.r_live, L.d_out, bwd);
  v.acc = factor_pair(L.acc_down, L.acc_up, acc_rank(L), L.d_out, bwd);
  v.W = L.acc_down, v.ldw = L.d_out;
  return v;
}
// one term on the r <= 64 chain kernels; h_only: the projection alone (Hsave), nothing written to Y
static ChainParams chain_params(const DirView& v, const Factors& f, void* Hsave, const void* bias, float scale, float beta,
                                bool h_only = false) {
  ChainParams p{};
  p.X = v.X, p.Y = h_only ? nullptr : v.Y, p.Hsave = Hsave, p.bias = bias;
  p.M = v.M, p.ldx = v.D1, p.ldy = v.D2, p.D1 = v.D1, p.D2 = h_only ? 0 : v.D2;
  p.F1b = f.F1, p.ldf1b = f.ld1, p.F2b = f.F2, p.ldf2b = f.ld2, p.rb = f.r;
  p.scale = scale, p.beta = beta;
  return p;
}
static ChainParams live_chain(const DirView& v, float beta, bool h_only = false) {
  return chain_params(v, v.live, v.H, h_only ? nullptr : v.bias, v.scale, beta, h_only);
}
// what the launches of one layer share: compute dtype, the layer's scratch (ws = NULL: none) under plan w, the stream
struct LayerRun {
  int dtype;
  char* ws;
  const WsPlan& w;
  size_t bytes;
  hipStream_t stream;
};

// One term of a wide-rank layer on the fused chain (chain_wide.hip), the factors packed into the workspace's wide region;
// SOW_ERR_UNSUPPORTED: nothing launched, the caller composes generic GEMMs (gemm_pair).  The scale goes where the saved
// projection wants it: the forward keeps H unscaled (the wide contract of h_save) and scales Y, the data gradient scales dh.
// rag: a term of an admitted ragged layer (rag_layer; the NO_WIDE_CHAIN switch does not apply); any other caller gets
// SOW_ERR_UNSUPPORTED for ragged widths, so that they keep the generic kernels.
static int wide_chain(const DirView& v, const Factors& f, void* Hsave, const void* bias, float scale, float beta,
                      const LayerRun& c, bool rag = false) {
  const bool ragged = v.D1 % 8 != 0 || v.D2 % 8 != 0;
  if ((ragged ? !rag : sw_on(SW_NO_WIDE_CHAIN)) || !c.ws || !c.w.wide_bytes || c.bytes < c.w.total + 255 ||
      chain_wide_pack_bytes(f.r, v.D1, v.D2) > c.w.wide_bytes)
    return SOW_ERR_UNSUPPORTED;
  WideArgs a{};
  a.X = v.X, a.Y = v.Y, a.F1 = f.F1, a.F2 = f.F2, a.ldf1 = f.ld1, a.ldf2 = f.ld2, a.Hsave = Hsave, a.bias = bias;
  a.M = v.M, a.D1 = v.D1, a.D2 = v.D2, a.r = f.r, a.hscale = v.bwd ? scale : 1.f, a.yscale = v.bwd ? 1.f : scale, a.beta = beta;
  a.bwd = v.bwd ? 1 : 0, a.pack = c.ws + c.w.off_wide, a.pack_bytes = c.w.wide_bytes;
  return launch_chain_wide(a, c.dtype, c.stream);
}
// the same term as two generic GEMMs:  h = X . F1 ;  Y = beta * Y + h . F2 + bias  (scaled as in wide_chain)
static int gemm_pair(const DirView& v, const Factors& f, void* h, const void* bias, float scale, float beta, const LayerRun& c) {
  int rc = launch_gemm(v.X, v.D1, false, f.F1, f.ld1, v.bwd, h, f.r, nullptr, v.M, f.r, v.D1, v.bwd ? scale : 1.f, 0.f, c.dtype,
                       c.stream);
  if (rc) return rc;
  return launch_gemm(h, f.r, false, f.F2, f.ld2, v.bwd, v.Y, v.D2, bias, v.M, v.D2, f.r, v.bwd ? 1.f : scale, beta, c.dtype,
                     c.stream);
}
// the operands of a fused low-rank-accumulator chain: one layer and direction, the factor pack in the flagged plan wf of ws
static WideAccArgs wide_acc_args(const DirView& v, char* ws, const WsPlan& wf) {
  WideAccArgs a{};
  a.X = v.X, a.Y = v.Y, a.Fa1 = v.acc.F1, a.Fl1 = v.live.F1, a.Fa2 = v.acc.F2, a.Fl2 = v.live.F2;
  a.ldfa1 = v.acc.ld1, a.ldfl1 = v.live.ld1, a.ldfa2 = v.acc.ld2, a.ldfl2 = v.live.ld2;
  a.Hsave = v.H, a.bias = v.bias, a.M = v.M, a.D1 = v.D1, a.D2 = v.D2, a.r_acc = v.acc.r, a.r_live = v.live.r;
  a.scale = v.scale, a.bwd = v.bwd ? 1 : 0, a.pack = ws + wf.off_wide, a.pack_bytes = wf.wide_bytes;
  return a;
}
// SOW_FUSE_ACC on an admitted call: the accumulator term and the live term of one direction as one chain
// (chain_wide_acc.hip), Y written once, H left as the two-pass path leaves it (the weight phases are the unflagged ones).
// SOW_ERR_UNSUPPORTED: nothing launched, the caller goes on with the unflagged path, unchanged.  The data gradient has no
// bias, and its H = dh lies in the workspace: the alignment tests on them are the forward's.
static int fused_acc_pass(const sow_layer_args& L, const DirView& v, const LayerRun& c) {
  if (sw_on(SW_NO_FUSED_ACC) || !c.ws || !al16p(v.X) || !al16p(v.Y) || !al16p(v.bias) || !al16p(v.H)) return SOW_ERR_UNSUPPORTED;
  const WsPlan wf = plan_of(L, c.dtype, SOW_FUSE_ACC);
  if (!wf.fused || c.bytes < wf.total + 255) return SOW_ERR_UNSUPPORTED;
  return launch_chain_wide_acc(wide_acc_args(v, c.ws, wf), c.dtype, c.stream);
}
// SOW_FUSE_ACC_DEEP on an admitted call (256 < r_acc + r_live <= 960): the same chain with H in column groups
// (chain_deep_acc.hip), in place of gemm_pair and the live chain with beta = 1.  Returns as fused_acc_pass does.
static int deep_acc_pass(const sow_layer_args& L, const DirView& v, const LayerRun& c) {
  if (sw_on(SW_NO_DEEP_ACC) || !c.ws || !al16p(v.X) || !al16p(v.Y) || !al16p(v.bias) || !al16p(v.H)) return SOW_ERR_UNSUPPORTED;
  const WsPlan wf = plan_of(L, c.dtype, SOW_FUSE_ACC_DEEP);
  if (!wf.deep || c.bytes < wf.total + 255) return SOW_ERR_UNSUPPORTED;
  return launch_chain_deep_acc(wide_acc_args(v, c.ws, wf), c.dtype, c.stream);
}
// The shared-input data gradient of siblings that all carry a low-rank accumulator (chain_shared_acc.hip): the admitted set
// of sow_backward_shared under SOW_FUSE_ACC (include/sow_amd.h).  `layers`: checked, one x, T, d_in and dx (shared_common,
// shared_fill_dx).  SOW_ERR_UNSUPPORTED and SOW_ERR_WORKSPACE: nothing launched, nothing written.
static int shared_fused_acc_data(const sow_layer_args* layers, int n, const Dtype& f, hipStream_t stream) {
  const int cd = f.cd;
  if (!f.fuse || (cd != SOW_BF16 && cd != SOW_F16) || sw_on(SW_NO_FUSED_ACC) || n > 4) return SOW_ERR_UNSUPPORTED;
  if (ceil_div(layers[0].T, 64) <= SHORT_NTB) return SOW_ERR_UNSUPPORTED;   // the streaming shared kernel's threshold
  int r_tot[4];
  for (int i = 0; i < n; ++i) {
    const sow_layer_args& L = layers[i];
    if (L.acc_kind != SOW_ACC_LOWRANK || !L.acc_up || !fused_acc_shape_ok(L.r_live, L.r_acc, L.d_in, L.d_out, cd))
      return SOW_ERR_UNSUPPORTED;
    r_tot[i] = L.r_acc + L.r_live;
  }
  if (!shared_acc_lds_ok(r_tot, n) || !al16p(layers[0].dx)) return SOW_ERR_UNSUPPORTED;
  for (int i = 0; i < n; ++i)
    if (!al16p(layers[i].dy)) return SOW_ERR_UNSUPPORTED;
  // below the unflagged plan no path runs the layer; between the two plans the grouped path does (the flag is a permission)
  for (int i = 0; i < n; ++i)
    if (layers[i].workspace_bytes < plan_of(layers[i], cd).total + 255) return SOW_ERR_WORKSPACE;
  WideAccArgs sib[4];
  for (int i = 0; i < n; ++i) {
    const sow_layer_args& L = layers[i];
    const WsPlan wf = plan_of(L, cd, SOW_FUSE_ACC);
    if (!wf.fused || L.workspace_bytes < wf.total + 255) return SOW_ERR_UNSUPPORTED;
    char* ws = ws_base(L.workspace);
    sib[i] = wide_acc_args(dir_view(L, true, ws + wf.off_dh), ws, wf);
  }
  return launch_chain_shared_acc(sib, n, layers[0].dx, layers[0].grad_beta, cd, stream);
}

// Dense accumulator, r_live <= 64: the product with the live term as a K-extension,  Y = [X, H] . [op(W); F2] + bias,
// H = scale * X . F1.  The operands of one layer and direction, as the one-launch kernels (gemm4h, gemm2h) take them:
static ProjGemm dense_args(const DirView& v) {
  return ProjGemm{v.X, v.W, v.live.F1, v.live.F2, v.Y, v.bias, v.H, v.M, v.D1, v.ldw, v.live.ld1, v.live.ld2, v.D2,
                  v.D2, v.D1, v.live.r, v.scale};
}
// Y = X . op(W) alone (the live term follows with beta = 1); rag: an admitted ragged layer
static int dense_product(const DirView& v, bool rag, int dtype, hipStream_t stream) {
  if (rag) return rag_dense_product(v.X, v.D1, v.W, v.ldw, v.bwd, v.Y, v.D2, v.M, v.D2, v.D1, dtype, stream);
  return gemm_auto(v.X, v.D1, v.W, v.ldw, v.bwd, v.Y, v.D2, nullptr, v.M, v.D2, v.D1, 1.f, 0.f, dtype, stream);
}
// The dense accumulator and the live term (r_live <= 64) as one product, one direction: gemm4h (projection pass + anti-phase
// main loop in one launch, the factors read in place), else gemm2h (one launch, H projected inside the GEMM, where the output
// spans at most two column tiles), else the two-launch composition: H (64 columns) from a chain launch, then the streaming
// kernel pick_gemm chooses with the extension operand E [ke rows of N].  *taken = false (and SOW_OK): none applies, nothing
// launched, the caller writes the dense product and the live term separately.
static int dense_ext_term(const sow_layer_args& L, const DirView& v, const LayerRun& c, bool* taken) {
  const ProjGemm g = dense_args(v);
  *taken = true;
  if (gemm4h_supported(g, v.bwd, c.dtype)) return launch_gemm4h(g, v.bwd, c.dtype, c.stream);
  if (gemm2h_supported(g, v.bwd, c.dtype)) return launch_gemm2h_group(&g, 1, v.bwd, c.stream);
  ChainParams ph = live_chain(v, 0.f, true);
  set_planes(ph, c.ws, c.w, c.bytes);
  // the extension operand: the forward reads B in place, the data gradient A zero-padded to 64 columns (workspace)
  void* apad = v.bwd ? c.ws + c.w.off_apad : nullptr;
  const void* E = v.bwd ? apad : L.B;
  const int64_t lde = v.bwd ? 64 : L.d_out;
  // the split-K scratch of the plan, where the workspace holds it
  const bool scratch = c.ws && c.bytes >= c.w.total;
  const bool sk = scratch && c.w.sk_bytes;
  void* const skp = sk ? c.ws + c.w.off_sk : nullptr;
  const size_t skb = sk ? c.w.sk_bytes : 0;
  // ke = r_live rows of B (forward), the 64 columns of the padded A (data gradient)
  const ExtGemm e{g.X, g.W, g.H, E, g.C, g.bias, g.M, g.ldx, g.ldw, 64, lde, g.ldc, g.N, g.K, v.bwd ? 64 : L.r_live, v.bwd, 1.f, 0.f};
  const GemmKernel k = chain2_supported(ph, c.dtype) ? pick_gemm(e, c.dtype, skp, skb) : GEMM_GENERIC;
  if (k == GEMM_GENERIC) {
    *taken = false;
    return SOW_OK;
  }
  // the padded A rides along in the dh launch when that grid is large enough
  const bool pad_fused = v.bwd && (int64_t)ceil_div(L.T, 64) * 64 >= L.d_in;
  if (pad_fused) ph.pad_src = L.A, ph.pad_dst = apad, ph.pad_rows = L.d_in, ph.pad_r = L.r_live;
  // short T: the H-only pass split over K (T / 64 workgroups cannot fill the chip: 29 us on 16 workgroups at 1024 x 4096);
  // launch_chain_short itself refuses longer inputs
  int rc = SOW_ERR_UNSUPPORTED;
  if (scratch) rc = launch_chain_short(ph, c.dtype, v.bwd, (float*)(c.ws + c.w.off_hp), c.stream);
  if (rc == SOW_ERR_UNSUPPORTED) rc = launch_chain2(ph, v.bwd, c.dtype, c.stream);
  if (rc) return rc;
  if (v.bwd && !pad_fused && (rc = launch_pad64(L.A, apad, L.d_in, L.r_live, c.stream))) return rc;
  return launch_picked(k, e, c.dtype, skp, skb, c.stream);
}

// An admitted ragged layer (rag_layer), one direction: the fused chain for the low-rank accumulator (scale 1) and for the
// live term, X read once per term; H holds the projection under the wide contract (forward: unscaled); a dense
// accumulator's product is written by gemm_rag first.
static int ragged_terms(const DirView& v, int acc_kind, const LayerRun& c) {
  int rc = SOW_OK;
  if (acc_kind == SOW_ACC_LOWRANK) rc = wide_chain(v, v.acc, nullptr, nullptr, 1.f, 0.f, c, true);
  if (acc_kind == SOW_ACC_DENSE) rc = dense_product(v, true, c.dtype, c.stream);
  if (rc) return rc;
  return wide_chain(v, v.live, v.H, v.bias, v.scale, acc_kind == SOW_ACC_NONE ? 0.f : 1.f, c, true);
}
// The low-rank accumulator term  Y = (X . F1) . F2  with the frozen factors, scale 1 (the live term follows with beta = 1):
// the r <= 64 chain kernel, or for a wide one the fused chain, else two generic GEMMs through the workspace.
static int lowrank_acc_term(const DirView& v, const LayerRun& c) {
  if (v.acc.r <= 64) {
    ChainParams p = chain_params(v, v.acc, nullptr, nullptr, 1.f, 0.f);
    set_planes(p, c.ws, c.w, c.bytes);
    return launch_chain(p, c.dtype, v.bwd, c.stream);
  }
  if (!c.ws || c.bytes < c.w.total) return SOW_ERR_WORKSPACE;   // the forward's check; a backward never gets here without
  const int rc = wide_chain(v, v.acc, nullptr, nullptr, 1.f, 0.f, c);
  return rc == SOW_ERR_UNSUPPORTED ? gemm_pair(v, v.acc, c.ws + c.w.off_t, nullptr, 1.f, 0.f, c) : rc;
}
// The live term of a wide-rank layer: the fused chain (H kept on chip, copied to v.H when given), else the generic
// composition with H in v.H or, for a forward without h_save, in the workspace.
static int wide_live_term(const DirView& v, float beta, const LayerRun& c) {
  const int rc = wide_chain(v, v.live, v.H, v.bias, v.scale, beta, c);
  if (rc != SOW_ERR_UNSUPPORTED) return rc;
  if (!v.H && !(c.ws && c.bytes >= c.w.total + 255)) return SOW_ERR_WORKSPACE;
  return gemm_pair(v, v.live, v.H ? v.H : c.ws + c.w.off_dh, v.bias, v.scale, beta, c);
}

// ---- weight gradients -----------------------------------------------------------------------------------------------
struct Phases {
  bool data, partial, reduce;
  bool weights() const { return partial || reduce; }
};
static inline Phases decode_phases(int phases) {
  return Phases{(phases & SOW_BWD_DATA) != 0, (phases & (SOW_BWD_WEIGHTS | SOW_BWD_WEIGHTS_PARTIAL)) != 0,
                (phases & (SOW_BWD_WEIGHTS | SOW_BWD_WEIGHTS_REDUCE)) != 0};
}
// The two slab-partial jobs of a layer with r_live <= 64: dA = x^T dh ; dB^T = dY^T h ; dbias = colsum(dY) via the all-ones
// column 63 (the chain kernels write 1.0 into column 63 of h_save / dh whenever r_live <= 63).
// vec: fp32 reads 16-byte vectors, the 16-bit dtypes 4-byte pairs.  The grouped launch takes 16-bit dtypes only
// (pick_tn never answers TN_DMA_WIDE for fp32), so the one rule serves it as it serves the single layer.
static TnParams tn_params(const sow_layer_args& L, const WsPlan& w, char* ws, int dtype) {
  TnParams tp{};
  tp.njobs = 2, tp.T = L.T, tp.ns = w.ns, tp.slab_len = w.slab_len;
  auto vec_ok = [&](const void* ptr, int D) {
    if (dtype == SOW_F32) return (D % 4 == 0 && al16p(ptr)) ? 1 : 0;
    return (D % 2 == 0 && al4p(ptr)) ? 1 : 0;
  };
  const bool ones_ok = L.dbias && L.r_live <= 63;
  tp.job[0] = TnJob{L.x, ws + w.off_dh, (float*)(ws + w.off_p0), (int64_t)L.d_in, L.d_in, -1, (L.d_in + 63) / 64,
                    vec_ok(L.x, L.d_in), 1};
  tp.job[1] = TnJob{L.dy, L.h_save, (float*)(ws + w.off_p1), (int64_t)L.d_out, L.d_out, ones_ok ? 63 : -1, (L.d_out + 63) / 64,
                    vec_ok(L.dy, L.d_out), 1};
  return tp;
}
// an operand of the row-owner kernel: job J of tn_params with its group-planned slabs (launch_tn_rows fills in the rest)
static TnRowsItem tn_rows_item(const TnJob& J, int64_t T, int ns, int slab_len) {
  return TnRowsItem{J.M, J.S, J.partial, J.ldm, T, J.D, 0, 0, 0, 0, ns, slab_len, 0};
}
// The wide-rank arm of the weight-gradient selector (r_live > 64; the rule: skinny_tn.hip).  w.pw_bytes != 0: plan_ws found
// tnw_shape_ok or an admitted ragged layer and the workspace holds the partials; what is left for launch_tn_wide to refuse is
// checked here, so the pick is what runs.
static TnKernel pick_tn_wide_rank(const sow_layer_args& L, const WsPlan& w, char* ws) {
  const bool rag = L.d_in % 8 != 0 || L.d_out % 8 != 0;
  if (!w.pw_bytes || sw_on(rag ? SW_NO_RAGGED : SW_NO_WIDE_CHAIN)) return TN_GEMM_PAIR;
  return tnw_operands_ok(L.x, ws + w.off_dh, L.dy, L.h_save, rag) ? TN_WIDE_RANK : TN_GEMM_PAIR;
}
// the kernel of layer L's PARTIAL phase (T > 0, plan w); *tp: its operands when r_live <= 64
static TnKernel pick_layer_tn(const sow_layer_args& L, const WsPlan& w, int dtype, TnParams* tp) {
  char* ws = ws_base(L.workspace);
  if (L.r_live > 64) return pick_tn_wide_rank(L, w, ws);
  *tp = tn_params(L, w, ws, dtype);
  return pick_tn(*tp, dtype);
}
// the reduction of the slab partials of one layer (shared by sow_backward_ex and the deferred, batched form)
static ReduceParams make_reduce_params(const WsPlan& w, char* ws, void* dA, void* dB, void* dbias_ones, int d_in, int d_out,
                                       int r_live, float grad_beta) {
  ReduceParams rp{};
  rp.njobs = 2, rp.ns = w.ns;
  rp.job[0] = ReduceJob{(const float*)(ws + w.off_p0), dA, nullptr, (int64_t)r_live, d_in, (d_in + 63) / 64 * 64, r_live, 0, -1,
                        1.f, grad_beta};
  rp.job[1] = ReduceJob{(const float*)(ws + w.off_p1), dB, dbias_ones, (int64_t)d_out, d_out, (d_out + 63) / 64 * 64, r_live, 1,
                        dbias_ones ? 63 : -1, 1.f /* h_save is already scaled */, grad_beta};
  rp.blocks0 = (d_in + 3) / 4;
  return rp;
}

size_t sow_reduce_desc_bytes(void) { return sizeof(ReduceParams); }

int sow_backward_reduce_desc(void* dA, void* dB, void* dbias, int64_t T, int d_in, int d_out, int r_live, int r_acc,
                             int acc_kind, float grad_beta, int dtype, void* workspace, size_t workspace_bytes, void* desc_out,
                             int* blocks_out) {
  if (acc_is_codes(acc_kind)) return SOW_ERR_UNSUPPORTED;
  const Dtype f = decode_dtype(dtype);   // the descriptor is the same with fp32 gradients: sow_reduce_batch picks the output type
  if (!f.layer_ok()) return SOW_ERR_DTYPE;
  if (T <= 0 || d_in <= 0 || d_out <= 0 || r_live <= 0) return SOW_ERR_SHAPE;
  if (!dA || !dB || !workspace || !desc_out || !blocks_out) return SOW_ERR_NULL;
  if (r_live > 64) {
    // the PARTIAL phase of a wide layer leaves finished gradients: an empty descriptor, no blocks in sow_reduce_batch
    memset(desc_out, 0, sizeof(ReduceParams));
    *blocks_out = 0;
    return SOW_OK;
  }
  if (dbias && r_live > 63) return SOW_ERR_UNSUPPORTED;   // no separate reduction: use SOW_BWD_WEIGHTS
  if (acc_kind != SOW_ACC_LOWRANK) r_acc = 0;
  const WsPlan w = plan_ws(T, d_in, d_out, r_live, r_acc, acc_kind, f.cd);
  if (workspace_bytes < w.total + 255) return SOW_ERR_WORKSPACE;
  const ReduceParams rp = make_reduce_params(w, ws_base(workspace), dA, dB, dbias, d_in, d_out, r_live, grad_beta);
  memcpy(desc_out, &rp, sizeof(rp));
  *blocks_out = (d_in + 3) / 4 + (d_out + 3) / 4;
  return SOW_OK;
}

int sow_reduce_batch(const void* descs, const int* starts, int n, int total_blocks, int dtype, void* stream) {
  const Dtype f = decode_dtype(dtype);
  if (!f.layer_ok()) return SOW_ERR_DTYPE;
  // the slab partials are fp32 whatever the compute dtype: fp32 gradients are their sums, rounded once.  An unflagged dtype
  // goes through as it came: SOW_FUSE_ACC is not stripped here, the launcher refuses it (SOW_ERR_DTYPE)
  const int gdt = f.param_f32 ? SOW_F32 : (dtype & ~SOW_ACC_NATIVE);
  if (n < 0 || total_blocks < 0) return SOW_ERR_SHAPE;
  if (n == 0) return SOW_OK;
  if (!descs || !starts) return SOW_ERR_NULL;
  return launch_tn_reduce_batch((const ReduceParams*)descs, starts, n, total_blocks, gdt, (hipStream_t)stream);
}

size_t sow_forward_workspace_bytes(int64_t T, int d_in, int d_out, int r_live, int r_acc, int acc_kind, int dtype) {
  const Dtype f = decode_dtype(dtype);
  if (acc_is_codes(acc_kind)) return 0;
  if (T < 0 || d_in <= 0 || d_out <= 0 || r_live <= 0 || !f.layer_ok()) return 0;
  if (f.param_f32) {   // the forward's own scratch (if any) followed by the packed parameters (pack_layer)
    const size_t own = sow_forward_workspace_bytes(T, d_in, d_out, r_live, r_acc, acc_kind, f.cd);
    const size_t pack = pack_bytes(d_in, d_out, r_live, acc_kind == SOW_ACC_LOWRANK ? r_acc : 0, acc_kind, f.native);
    return own ? own + pack : pack + 256;
  }
  const bool wide_acc = acc_kind == SOW_ACC_LOWRANK && r_acc > 64;
  const WsPlan w = plan_ws(T, d_in, d_out, r_live, r_acc, acc_kind, f.cd, f.perm());
  if (!w.fused && !w.deep && !wide_acc && r_live <= 64 && short_hp_bytes(T, d_in, d_out, r_live, f.cd) == 0 && w.planes_bytes == 0 && w.sk_bytes == 0)
    return 0;   // the forward does not touch it
  return w.total + 256;
}

size_t sow_workspace_bytes(int64_t T, int d_in, int d_out, int r_live, int r_acc, int acc_kind, int dtype) {
  const Dtype f = decode_dtype(dtype);
  if (acc_is_codes(acc_kind)) return 0;
  if (T < 0 || d_in <= 0 || d_out <= 0 || r_live <= 0 || !f.layer_ok()) return 0;
  const size_t pack = f.param_f32 ? pack_bytes(d_in, d_out, r_live, acc_kind == SOW_ACC_LOWRANK ? r_acc : 0, acc_kind, f.native) : 0;
  return plan_ws(T, d_in, d_out, r_live, r_acc, acc_kind, f.cd, f.perm()).total + pack + 256;
}

// ---- single layer -----------------------------------------------------------------------------------------------------
static int forward_impl(const sow_layer_args& L, int dtype, int perm, hipStream_t stream) {
  if (!ok_dtype(dtype)) return SOW_ERR_DTYPE;
  int rc = check_layer(L, false, true);
  if (rc || L.T == 0) return rc;
  const int r_live = L.r_live, r_acc = acc_rank(L), acc_kind = L.acc_kind;
  const size_t workspace_bytes = L.workspace_bytes;
  const WsPlan w = plan_of(L, dtype);
  char* ws = L.workspace ? ws_base(L.workspace) : nullptr;
  const DirView v = dir_view(L, false, nullptr);
  const LayerRun c{dtype, ws, w, workspace_bytes, stream};
  float beta = 0.f;
  if ((perm & SOW_FUSE_ACC) && (rc = fused_acc_pass(L, v, c)) != SOW_ERR_UNSUPPORTED) return rc;
  if ((perm & SOW_FUSE_ACC_DEEP) && (rc = deep_acc_pass(L, v, c)) != SOW_ERR_UNSUPPORTED) return rc;
  // ragged widths; without workspace or with views off 16 bytes, the generic kernels below
  if (rag_layer(r_live, r_acc, acc_kind, L.d_in, L.d_out, dtype) && !sw_on(SW_NO_RAGGED) && ws &&
      workspace_bytes >= w.total + 255 && al16p(L.x) && al16p(L.y) && (!L.bias || al16p(L.bias)) &&
      (!L.h_save || al4p(L.h_save)))
    return ragged_terms(v, acc_kind, c);
  if (acc_kind == SOW_ACC_DENSE) {
    if (r_live <= 64 && L.h_save) {
      // one product with the low-rank term as a K-extension:  y = [x, h] . [W_acc; B] + bias,  h = scale * x . A
      bool taken;
      rc = dense_ext_term(L, v, c, &taken);
      if (taken) return rc;
    }
    rc = dense_product(v, false, dtype, stream);
    if (rc) return rc;
    beta = 1.f;
  } else if (acc_kind == SOW_ACC_LOWRANK) {
    if ((rc = lowrank_acc_term(v, c))) return rc;
    beta = 1.f;
  }
  if (r_live <= 64) {
    ChainParams p = live_chain(v, beta);
    set_planes(p, ws, w, workspace_bytes);
    if (ws && workspace_bytes >= w.total) {
      rc = launch_chain_short(p, dtype, false, (float*)(ws + w.off_hp), stream);
      if (rc != SOW_ERR_UNSUPPORTED) return rc;
    }
    return launch_chain(p, dtype, false, stream);
  }
  // wide rank:  h = x A ; y = beta*y + scale * h B + bias
  return wide_live_term(v, beta, c);
}

int sow_forward(const void* x, const void* A, const void* B, const void* acc_down, const void* acc_up, const void* bias,
                void* y, void* h_save, int64_t T, int d_in, int d_out, int r_live, int r_acc, int acc_kind, float scale,
                int dtype, void* workspace, size_t workspace_bytes, void* stream) {
  if (acc_is_codes(acc_kind)) return SOW_ERR_UNSUPPORTED;
  const Dtype f = decode_dtype(dtype);
  if (!f.layer_ok()) return SOW_ERR_DTYPE;
  sow_layer_args L = single_layer(x, A, B, acc_down, acc_up, bias, y, h_save, nullptr, nullptr, nullptr, nullptr, nullptr, T, d_in,
                                  d_out, r_live, r_acc, acc_kind, scale, 0.f, workspace, workspace_bytes);
  if (f.param_f32 && T > 0) {   // fp32 parameters: forward_impl's checks before the pack launch reads them
    const int rc = pack_single(L, f.cd, true, f.native, (hipStream_t)stream);
    if (rc) return rc;
  }
  return forward_impl(L, f.cd, f.perm(), (hipStream_t)stream);
}

// gdt: the dtype of dA / dB / dbias -- dtype, or SOW_F32 under SOW_PARAM_F32 (the fp32 slab sums rounded once to fp32)
static int backward_impl(const sow_layer_args& L, int dtype, int gdt, int phases, int perm, hipStream_t stream) {
  const Phases ph = decode_phases(phases);
  bool do_data = ph.data;
  if (!ph.data && !ph.weights()) return SOW_ERR_SHAPE;
  if (!ok_dtype(dtype)) return SOW_ERR_DTYPE;
  int rc = check_layer(L, true, true);
  if (rc) return rc;
  const int64_t T = L.T;
  const int d_in = L.d_in, d_out = L.d_out, r_live = L.r_live, r_acc = acc_rank(L), acc_kind = L.acc_kind;
  if (T == 0) {
    // empty batch: gradients are zero (or unchanged when accumulating); x / dy / dx may be NULL
    if (!L.dA || !L.dB) return SOW_ERR_NULL;
    if (L.grad_beta == 0.f) {
      void* ptrs[3] = {L.dA, L.dB, L.dbias};
      int64_t bytes[3] = {(int64_t)d_in * r_live * (int64_t)esize(gdt), (int64_t)r_live * d_out * (int64_t)esize(gdt),
                          L.dbias ? (int64_t)d_out * (int64_t)esize(gdt) : 0};
      return launch_multi_zero(ptrs, bytes, 3, stream);
    }
    return SOW_OK;
  }
  const size_t workspace_bytes = L.workspace_bytes;
  const WsPlan w = plan_of(L, dtype);
  if (workspace_bytes < w.total + 255) return SOW_ERR_WORKSPACE;
  char* ws = ws_base(L.workspace);
  void* dh = ws + w.off_dh;
  const DirView v = dir_view(L, true, dh);
  const LayerRun c{dtype, ws, w, workspace_bytes, stream};
  float beta = 0.f;
  bool data_done = false;
  if (do_data && (perm & SOW_FUSE_ACC)) {
    rc = fused_acc_pass(L, v, c);
    if (rc && rc != SOW_ERR_UNSUPPORTED) return rc;
    if (!rc) do_data = false;
  }
  if (do_data && (perm & SOW_FUSE_ACC_DEEP)) {
    rc = deep_acc_pass(L, v, c);
    if (rc && rc != SOW_ERR_UNSUPPORTED) return rc;
    if (!rc) do_data = false;
  }
  // ragged widths: the fused chain for the data gradient (dY and dX views 16-byte aligned, else the generic kernels below:
  // they leave the same dh) and skinny_tn_wide for every weight gradient, dbias included, in the PARTIAL phase
  const bool rag_w = rag_layer(r_live, r_acc, acc_kind, d_in, d_out, dtype) && !sw_on(SW_NO_RAGGED);
  if (rag_w && do_data && al16p(L.dy) && al16p(L.dx)) {
    if ((rc = ragged_terms(v, acc_kind, c))) return rc;
    do_data = false;
  }
  if (!do_data) {
    // weights-only call: dh was produced by an earlier SOW_BWD_DATA call on the same workspace
  } else if (acc_kind == SOW_ACC_DENSE) {
    if (r_live <= 64) {
      // one product with the low-rank term as a K-extension:  dX = [dY, dh] . [W_acc^T; A^T],  dh = scale * dY . B^T
      // (in the one-launch kernels dh is projected by the kernel itself, A^T read from A's own 2r-byte rows)
      if ((rc = dense_ext_term(L, v, c, &data_done))) return rc;
    }
    // dX = dY . W_acc^T   (W_acc stored [d_in, d_out] = [N, K])
    if (!data_done) rc = dense_product(v, false, dtype, stream);
    if (rc) return rc;
    beta = 1.f;
  } else if (acc_kind == SOW_ACC_LOWRANK) {
    if ((rc = lowrank_acc_term(v, c))) return rc;   // dX = (dY . R_up^T) . Q^T
    beta = 1.f;
  }
  if (r_live <= 64) {
    ChainParams p = live_chain(v, beta);
    set_planes(p, ws, w, workspace_bytes);
    if (do_data && !data_done) {
      rc = launch_chain_short(p, dtype, true, short_hp_bytes(T, d_in, d_out, r_live, dtype) ? (float*)(ws + w.off_hp) : nullptr, stream);
      if (rc == SOW_ERR_UNSUPPORTED) rc = launch_chain(p, dtype, true, stream);
      if (rc) return rc;
    }
    if (!ph.weights()) return SOW_OK;
    const bool ones_ok = L.dbias && r_live <= 63;
    if (ph.partial) {
      rc = launch_tn(tn_params(L, w, ws, dtype), dtype, stream);
      if (rc) return rc;
    }
    if (!ph.reduce) return SOW_OK;
    const ReduceParams rp = make_reduce_params(w, ws, L.dA, L.dB, ones_ok ? L.dbias : nullptr, d_in, d_out, r_live, L.grad_beta);
    rc = launch_tn_reduce(rp, gdt, stream);
    if (rc) return rc;
    if (L.dbias && !ones_ok) {
      rc = launch_colsum(L.dy, T, d_out, L.dbias, L.grad_beta, dtype, gdt, stream);
      if (rc) return rc;
    }
    return SOW_OK;
  }
  // wide rank: the fused chain (dh = scale dY B^T to the workspace, dX = beta dX + dh A^T) and the token-slab weight-gradient
  // kernel, else the generic GEMM composition
  if (do_data && (rc = wide_live_term(v, beta, c))) return rc;
  if (!ph.partial) return SOW_OK;   // wide ranks: the PARTIAL phase does all of the weight gradients
  if (pick_tn_wide_rank(L, w, ws) == TN_WIDE_RANK)
    return launch_tn_wide(L.x, dh, L.dy, L.h_save, L.dA, L.dB, L.dbias, T, d_in, d_out, r_live, L.scale, L.grad_beta, dtype, gdt,
                          ws + w.off_pw, w.pw_bytes, stream);
  rc = launch_gemm_out(L.x, d_in, true, dh, r_live, false, L.dA, r_live, nullptr, d_in, r_live, (int)T, 1.f, L.grad_beta, dtype, gdt,
                       stream);
  if (rc) return rc;
  rc = launch_gemm_out(L.h_save, r_live, true, L.dy, d_out, false, L.dB, d_out, nullptr, r_live, d_out, (int)T, L.scale, L.grad_beta,
                       dtype, gdt, stream);
  if (rc) return rc;
  if (L.dbias) {
    rc = launch_colsum(L.dy, T, d_out, L.dbias, L.grad_beta, dtype, gdt, stream);
    if (rc) return rc;
  }
  return SOW_OK;
}

int sow_backward_ex(const void* dy, const void* x, const void* h_save, const void* A, const void* B, const void* acc_down,
                    const void* acc_up, void* dx, void* dA, void* dB, void* dbias, int64_t T, int d_in, int d_out,
                    int r_live, int r_acc, int acc_kind, float scale, float grad_beta, int dtype, void* workspace,
                    size_t workspace_bytes, int phases, void* stream) {
  if (acc_is_codes(acc_kind)) return SOW_ERR_UNSUPPORTED;
  const Dtype f = decode_dtype(dtype);
  sow_layer_args L = single_layer(x, A, B, acc_down, acc_up, nullptr, nullptr, const_cast<void*>(h_save), dy, dx, dA, dB, dbias, T,
                                  d_in, d_out, r_live, r_acc, acc_kind, scale, grad_beta, workspace, workspace_bytes);
  if (f.native_bit && !f.layer_ok()) return SOW_ERR_DTYPE;
  if (!f.param_f32) return backward_impl(L, f.cd, f.cd, phases, f.perm(), (hipStream_t)stream);
  if (!f.layer_ok()) return SOW_ERR_DTYPE;
  // fp32 parameters: only the data gradient reads the factors (and the accumulator); they are packed when it runs
  if ((phases & SOW_BWD_DATA) && T > 0) {
    const int rc = pack_single(L, f.cd, false, f.native, (hipStream_t)stream);
    if (rc) return rc;
  }
  return backward_impl(L, f.cd, SOW_F32, phases, 0, (hipStream_t)stream);
}

int sow_backward(const void* dy, const void* x, const void* h_save, const void* A, const void* B, const void* acc_down,
                 const void* acc_up, void* dx, void* dA, void* dB, void* dbias, int64_t T, int d_in, int d_out,
                 int r_live, int r_acc, int acc_kind, float scale, float grad_beta, int dtype, void* workspace,
                 size_t workspace_bytes, void* stream) {
  return sow_backward_ex(dy, x, h_save, A, B, acc_down, acc_up, dx, dA, dB, dbias, T, d_in, d_out, r_live, r_acc, acc_kind,
                         scale, grad_beta, dtype, workspace, workspace_bytes, SOW_BWD_DATA | SOW_BWD_WEIGHTS, stream);
}

// ---- grouped entry points ------------------------------------------------------------------------------------
// A group is n INDEPENDENT SoWLinear calls (e.g. q / k / v of one attention block, gate / up of one MLP).  Layers that
// take the plain bf16 / f16 streaming kernels (no accumulator, r <= 64, T / 64 > SHORT_NTB) share launches, C2_MAXG /
// TN_MAXG at a time; every other layer is forwarded to the single-layer path.  Results are bit-identical to n
// separate calls: the shared grid runs each layer's own workgroups unchanged.
// w: the layer's plan (data gradient only: dh lies in the workspace)
static bool group_chain_params(const sow_layer_args& L, bool bwd, int dtype, const WsPlan& w, ChainParams* out) {
  if ((dtype != SOW_BF16 && dtype != SOW_F16) || L.acc_kind != SOW_ACC_NONE || L.r_live > 64 || sw_on(SW_NO_GROUPED) || sw_on(SW_FORCE_CHAIN_V1))
    return false;
  if (ceil_div(L.T, 64) <= SHORT_NTB) return false;   // short inputs: K / column split, single-layer path
  const ChainParams p = live_chain(dir_view(L, bwd, bwd ? ws_base(L.workspace) + w.off_dh : nullptr), 0.f);
  if (!chain2_supported(p, dtype)) return false;
  // the alignment conditions launch_chain2 would reject (it then falls back inside launch_chain)
  if (!al16p(L.B) || L.d_out % 8 || !al4p(L.A)) return false;
  *out = p;
  return true;
}

// Group-planned slab counts for the weight-gradient partial sums (skinny_tn.hip: tn_partial_rows_kernel).  A pure function
// of the layer list, so that sow_backward_group and sow_backward_group_reduce_desc agree.  Items 2 i, 2 i + 1 = the two
// operands (x with dh, dY with h) of layer i.
// f16 takes the plan only when the caller asks for it (SOW_BWD_GROUP_SLABS: a deferred reduction); a call that runs both
// weight phases itself keeps the column-owner kernel for f16, whose grouped results are pinned bit-identical to single calls.
static bool group_rows_plan(const sow_layer_args* layers, int n, int dtype, int phases, int* ns, int* slab_len) {
  // (the 16-bit dtypes while they take the wide LDS-DMA kernel: not f16 under NO_F16_TN, neither under TN_NARROW)
  if (tn_shape_kernel(0, 0, 0, dtype) != TN_DMA_WIDE || (dtype == SOW_F16 && !(phases & SOW_BWD_GROUP_SLABS)) || n < 1 || n > TN_MAXG)
    return false;
  int64_t T[TNR_MAXI];
  int D[TNR_MAXI], cap[TNR_MAXI];
  for (int i = 0; i < n; ++i) {
    const sow_layer_args& L = layers[i];
    if (L.T <= 0 || L.r_live > 64 || (L.dbias && L.r_live > 63)) return false;
    const WsPlan w = plan_of(L, dtype);
    if (L.workspace_bytes < w.total + 255) return false;
    const TnParams tp = tn_params(L, w, ws_base(L.workspace), dtype);
    if (!tn_operand_ok(tp.job[0], 8) || !tn_operand_ok(tp.job[1], 8)) return false;
    T[2 * i] = T[2 * i + 1] = L.T;
    D[2 * i] = L.d_in, D[2 * i + 1] = L.d_out;
    cap[2 * i] = cap[2 * i + 1] = w.ns_cap;
  }
  return tn_rows_plan(T, D, cap, 2 * n, ns, slab_len);
}
// What sow_backward_group does and sow_backward_group_plan reports: the row-owner weight-gradient kernel with slab counts
// planned over the group, when the caller asks for it (and then builds the deferred reduction from
// sow_backward_group_reduce_desc), or when the call runs the reduction itself.
static bool group_rows(const sow_layer_args* layers, int n, int dtype, int phases, int* rns, int* rslab) {
  const Phases ph = decode_phases(phases);
  return ph.weights() && ((phases & SOW_BWD_GROUP_SLABS) || (ph.partial && ph.reduce)) &&
         group_rows_plan(layers, n, dtype, phases, rns, rslab);
}

// fp32 parameters of a group: a copy of the layer list pointing at the packed operands, every layer packed by ONE launch
static int pack_group(const sow_layer_args* layers, int n, int cd, bool bwd, bool native, std::vector<sow_layer_args>& out,
                      hipStream_t stream) {
  out.assign(layers, layers + n);
  std::vector<PackItem> items;
  int rc;
  for (sow_layer_args& L : out) {
    if ((rc = check_layer(L, bwd, true))) return rc;
    if (L.T == 0) continue;
    normalise_acc(L);
    if (bwd) L.bias = nullptr;   // backward reads no bias
    if ((rc = pack_layer(L, cd, !bwd, native, items))) return rc;
  }
  return launch_pack_params(items.data(), (int)items.size(), cd, stream);
}

static int forward_group_impl(const sow_layer_args* layers, int n, int dtype, int perm, hipStream_t stream) {
  if (!ok_dtype(dtype)) return SOW_ERR_DTYPE;
  if (n < 0) return SOW_ERR_SHAPE;
  if (n == 0) return SOW_OK;
  if (!layers) return SOW_ERR_NULL;
  ChainParams batch[C2_MAXG];
  ProjGemm gbatch[4];
  int nb = 0, ng = 0, rc;
  for (int i = 0; i < n; ++i) {
    const sow_layer_args& L = layers[i];
    if ((rc = check_layer(L, false, false))) return rc;
    if (L.T == 0) continue;
    if (group_chain_params(L, false, dtype, WsPlan{}, &batch[nb])) {   // h_save may be NULL (no backward follows)
      if (++nb == C2_MAXG) {
        if ((rc = launch_chain2_group(batch, nb, false, dtype, stream))) return rc;
        nb = 0;
      }
      continue;
    }
    if (L.acc_kind == SOW_ACC_DENSE && L.r_live <= 64 && L.h_save) {
      const ProjGemm g = dense_args(dir_view(L, false, nullptr));
      // dense accumulator: gemm4h (one launch per layer) where it applies
      if (gemm4h_supported(g, false, dtype)) {
        if ((rc = launch_gemm4h(g, false, dtype, stream))) return rc;
        continue;
      }
      // dense accumulator, one launch per layer (gemm2h): the layers of a group share the grid
      if (!sw_on(SW_NO_GROUPED) && gemm2h_supported(g, false, dtype)) {
        gbatch[ng] = g;
        if (++ng == 4) {
          if ((rc = launch_gemm2h_group(gbatch, ng, false, stream))) return rc;
          ng = 0;
        }
        continue;
      }
    }
    if ((rc = forward_impl(L, dtype, perm, stream))) return rc;
  }
  if (ng && (rc = launch_gemm2h_group(gbatch, ng, false, stream))) return rc;
  return nb ? launch_chain2_group(batch, nb, false, dtype, stream) : SOW_OK;
}

int sow_forward_group(const sow_layer_args* layers, int n, int dtype, void* stream) {
  if (any_codes_acc(layers, n)) return SOW_ERR_UNSUPPORTED;
  const Dtype f = decode_dtype(dtype);
  if (!f.layer_ok()) return SOW_ERR_DTYPE;
  if (!f.param_f32 || n <= 0 || !layers) return forward_group_impl(layers, n, f.cd, f.perm(), (hipStream_t)stream);
  std::vector<sow_layer_args> packed;
  const int rc = pack_group(layers, n, f.cd, false, f.native, packed, (hipStream_t)stream);
  return rc ? rc : forward_group_impl(packed.data(), n, f.cd, 0, (hipStream_t)stream);
}

// ---- generation-sized forwards (skinny_fwd.hip) --------------------------------------------------------------
// The admitted set, decided from the shape alone: 1 <= T <= 32, bf16 / f16 (SOW_PARAM_F32 only with SOW_ACC_NATIVE), a dense accumulator (in the
// compute dtype, as E4M3 codes or as MXFP4 codes) or none, r_live <= 64, widths multiples of 8 (d_in of 32 for MXFP4: whole blocks).
// (tmax: 32 for sow_forward_skinny, SOW_SKINNY_ROWS_MAX for sow_forward_skinny_rows)
static bool skinny_shape_ok(int64_t T, int d_in, int d_out, int r_live, int acc_kind, int dtype, int tmax = 32) {
  return (dtype == SOW_BF16 || dtype == SOW_F16) && T >= 1 && T <= tmax && d_in > 0 && d_out > 0 && r_live >= 1 && r_live <= 64 &&
         acc_kind_known(acc_kind) && acc_kind != SOW_ACC_LOWRANK && d_in % 8 == 0 && d_out % 8 == 0 && (acc_kind != SOW_ACC_DENSE_FP4 || d_in % 32 == 0);
}
struct SkWs {
  size_t off_py, off_ph, total;
};
static SkWs skinny_ws(int64_t T, int d_in, int d_out, int acc_kind) {
  int S, KS, ncr;
  skinny_rows_plan(T, d_in, d_out, acc_kind, &S, &KS, &ncr);   // skinny_plan itself for T <= 32
  SkWs w;
  w.off_py = 0;
  w.off_ph = acc_kind != SOW_ACC_NONE ? al256(skinny_py_bytes(T, d_out, S)) : 0;
  w.total = 256 + w.off_ph + al256(skinny_ph_bytes(T, S));
  return w;
}

static size_t skinny_ws_query(int64_t T, int d_in, int d_out, int r_live, int acc_kind, int dtype, int tmax = 32) {
  const Dtype f = decode_dtype(dtype);
  if ((f.param_f32 && !f.native) || !skinny_shape_ok(T, d_in, d_out, r_live, acc_kind, f.cd, tmax)) return 0;
  return skinny_ws(T, d_in, d_out, acc_kind).total;
}

// (a quantised accumulator has the query of its format: this one keeps answering 0 for every kind value it answered 0 for before)
size_t sow_forward_skinny_workspace_bytes(int64_t T, int d_in, int d_out, int r_live, int acc_kind, int dtype) {
  return acc_is_codes(acc_kind) ? 0 : skinny_ws_query(T, d_in, d_out, r_live, acc_kind, dtype);
}
size_t sow_forward_skinny_fp8_workspace_bytes(int64_t T, int d_in, int d_out, int r_live, int dtype) {
  return skinny_ws_query(T, d_in, d_out, r_live, SOW_ACC_DENSE_FP8, dtype);
}
size_t sow_forward_skinny_fp4_workspace_bytes(int64_t T, int d_in, int d_out, int r_live, int dtype) {
  return skinny_ws_query(T, d_in, d_out, r_live, SOW_ACC_DENSE_FP4, dtype);
}
// one query for all four kinds and 1 <= T <= SOW_SKINNY_ROWS_MAX; for T <= 32 what the matching query above returns
size_t sow_forward_skinny_rows_workspace_bytes(int64_t T, int d_in, int d_out, int r_live, int acc_kind, int dtype) {
  return skinny_ws_query(T, d_in, d_out, r_live, acc_kind, dtype, SOW_SKINNY_ROWS_MAX);
}

// The checks of this entry point are its own (not check_layer): stricter, and every layer is checked before the first
// launch, so that a refusal leaves all outputs and workspaces untouched.
static int forward_skinny_impl(const sow_layer_args* layers, int n, int dtype, void* stream, int tmax) {
  const Dtype f = decode_dtype(dtype);
  const int cd = f.cd;
  if (!f.layer_ok() || cd == SOW_F32) return SOW_ERR_DTYPE;
  // fp32 factors are admitted over a native accumulator only (SOW_ACC_NATIVE: the kernels round A, B and the bias in registers)
  if ((f.param_f32 && !f.native) || sw_on(SW_NO_SKINNY)) return SOW_ERR_UNSUPPORTED;
  if (n < 0) return SOW_ERR_SHAPE;
  if (n == 0) return SOW_OK;
  if (!layers) return SOW_ERR_NULL;
  if (n > SK_MAXL) return SOW_ERR_UNSUPPORTED;
  SkLayer sk[SK_MAXL];
  int m = 0, call_kind = SOW_ACC_NONE;      // the kind of the call's dense accumulators, once one was seen
  for (int i = 0; i < n; ++i) {
    const sow_layer_args& L = layers[i];
    if (L.T < 0 || L.d_in <= 0 || L.d_out <= 0 || L.r_live <= 0) return SOW_ERR_SHAPE;
    if (!acc_kind_known(L.acc_kind)) return SOW_ERR_SHAPE;
    if (L.T == 0) continue;
    if (!skinny_shape_ok(L.T, L.d_in, L.d_out, L.r_live, L.acc_kind, cd, tmax)) return SOW_ERR_UNSUPPORTED;
    const bool codes = acc_is_codes(L.acc_kind), fp4 = L.acc_kind == SOW_ACC_DENSE_FP4;
    const bool dense = L.acc_kind == SOW_ACC_DENSE || codes;
    if (!L.x || !L.A || !L.B || !L.y || (dense && !L.acc_down) || (codes && !L.acc_up)) return SOW_ERR_NULL;
    if (!al16p(L.x) || !al16p(L.y) || !al16p(L.A) || !al16p(L.B) || !al16p(L.bias) || (dense && !fp4 && !al16p(L.acc_down)))
      return SOW_ERR_UNSUPPORTED;
    // MXFP4: codes and block scales are read in 8-byte pieces
    if (fp4 && ((reinterpret_cast<uintptr_t>(L.acc_down) | reinterpret_cast<uintptr_t>(L.acc_up)) & 7)) return SOW_ERR_UNSUPPORTED;
    // one kind of dense accumulator per call (the kernels are instantiated per kind)
    if (dense && call_kind != SOW_ACC_NONE && call_kind != L.acc_kind) return SOW_ERR_UNSUPPORTED;
    if (dense) call_kind = L.acc_kind;
    const SkWs w = skinny_ws(L.T, L.d_in, L.d_out, L.acc_kind);
    if (!L.workspace || L.workspace_bytes < w.total) return SOW_ERR_WORKSPACE;
    char* ws = ws_base(L.workspace);
    SkLayer& K = sk[m++];
    K = SkLayer{};
    K.x = L.x, K.W = dense ? L.acc_down : nullptr, K.A = L.A, K.B = L.B, K.bias = L.bias, K.y = L.y;
    K.Py = dense ? (float*)(ws + w.off_py) : nullptr, K.Ph = (float*)(ws + w.off_ph);
    K.T = (int)L.T, K.d_in = L.d_in, K.d_out = L.d_out, K.r = L.r_live, K.scale = L.scale;
    K.wexp = codes ? (const int8_t*)L.acc_up : nullptr;
  }
  // layers of at most 32 rows keep the plan and the kernels of sow_forward_skinny, layers past 32 take the four-row-tile forms:
  // two launches each (a call of one range launches nothing for the other)
  SkLayer hi[SK_MAXL];
  int nlo = 0, nhi = 0;
  for (int i = 0; i < m; ++i) {
    if (sk[i].T > 32) hi[nhi++] = sk[i];
    else sk[nlo++] = sk[i];
  }
  const int kind = call_kind != SOW_ACC_NONE ? call_kind : SOW_ACC_DENSE;
  const int rc = launch_skinny_fwd(sk, nlo, cd, kind, f.native, (hipStream_t)stream);
  return rc ? rc : launch_skinny_fwd(hi, nhi, cd, kind, f.native, (hipStream_t)stream, true);
}
int sow_forward_skinny(const sow_layer_args* layers, int n, int dtype, void* stream) {
  return forward_skinny_impl(layers, n, dtype, stream, 32);
}
int sow_forward_skinny_rows(const sow_layer_args* layers, int n, int dtype, void* stream) {
  return forward_skinny_impl(layers, n, dtype, stream, SOW_SKINNY_ROWS_MAX);
}

// ---- short batches of dense-accumulator layers (skinny_fwd.hip: the row-block forms) ------------------------------------
// The admitted set, from the shape alone: bf16 / f16 without flags, SOW_ACC_DENSE, 1 <= T <= SOW_SHORT_ROWS_MAX, r_live <= 64,
// widths multiples of 8.
static_assert(SOW_SHORT_ROWS_MAX == SK_SHORT_MAX && SOW_SHORT_ROWS_MAX == 64 * SK_MAXL, "a layer's row blocks are one launch group");
static bool short_shape_ok(int64_t T, int d_in, int d_out, int r_live, int acc_kind, int dtype) {
  return (dtype == SOW_BF16 || dtype == SOW_F16) && acc_kind == SOW_ACC_DENSE && T >= 1 && T <= SOW_SHORT_ROWS_MAX && d_in > 0 && d_out > 0 &&
         r_live >= 1 && r_live <= 64 && d_in % 8 == 0 && d_out % 8 == 0;
}
// the slab partials of one direction: Py [S][T][N] (row block b at S * 64 b * N floats), then Ph [S][T][64], each 256-aligned
struct ShortWs {
  int S, KS, ncr;
  size_t off_ph, bytes;
};
static ShortWs short_ws(int64_t T, int K, int N, bool bwd) {
  ShortWs w;
  short_rows_plan(T, K, N, bwd ? SK_SHORT_KQ_BWD : SK_SHORT_KQ_FWD, &w.S, &w.KS, &w.ncr);
  w.off_ph = al256(skinny_py_bytes(T, N, w.S));
  w.bytes = w.off_ph + al256(skinny_ph_bytes(T, w.S));
  return w;
}
static bool short_dtype_ok(const Dtype& f) { return !f.param_f32 && !f.native_bit && (f.cd == SOW_BF16 || f.cd == SOW_F16); }

size_t sow_forward_short_workspace_bytes(int64_t T, int d_in, int d_out, int r_live, int acc_kind, int dtype) {
  const Dtype f = decode_dtype(dtype);
  if (!short_dtype_ok(f) || !short_shape_ok(T, d_in, d_out, r_live, acc_kind, f.cd)) return 0;
  return 256 + short_ws(T, d_in, d_out, false).bytes;
}
// the plan of sow_workspace_bytes (dh at off_dh, the weight phases' partials), then the slab partials of the larger direction:
// the forward puts its own at the front of whichever workspace it is given (nothing there is live before the data phase)
size_t sow_short_workspace_bytes(int64_t T, int d_in, int d_out, int r_live, int acc_kind, int dtype) {
  const Dtype f = decode_dtype(dtype);
  if (!short_dtype_ok(f) || !short_shape_ok(T, d_in, d_out, r_live, acc_kind, f.cd)) return 0;
  const size_t fw = short_ws(T, d_in, d_out, false).bytes, bw = short_ws(T, d_out, d_in, true).bytes;
  return plan_ws(T, d_in, d_out, r_live, 0, SOW_ACC_DENSE, f.cd).total + (fw > bw ? fw : bw) + 256;
}

// Checks of their own, as sow_forward_skinny: every layer is checked before the first launch.
static int short_impl(const sow_layer_args* layers, int n, int dtype, void* stream, bool bwd) {
  const Dtype f = decode_dtype(dtype);
  const int cd = f.cd;
  if (!f.layer_ok() || cd == SOW_F32) return SOW_ERR_DTYPE;
  if (f.param_f32 || f.native_bit || sw_on(SW_NO_SKINNY)) return SOW_ERR_UNSUPPORTED;
  if (n < 0) return SOW_ERR_SHAPE;
  if (n == 0) return SOW_OK;
  if (!layers) return SOW_ERR_NULL;
  if (n > SK_MAXL) return SOW_ERR_UNSUPPORTED;
  for (int i = 0; i < n; ++i)
    if (layers[i].acc_kind != SOW_ACC_DENSE) return acc_kind_known(layers[i].acc_kind) ? SOW_ERR_UNSUPPORTED : SOW_ERR_SHAPE;
  std::vector<SkLayer> e;
  for (int i = 0; i < n; ++i) {
    const sow_layer_args& L = layers[i];
    if (L.T < 0 || L.d_in <= 0 || L.d_out <= 0 || L.r_live <= 0) return SOW_ERR_SHAPE;
    if (L.T == 0) continue;
    if (!short_shape_ok(L.T, L.d_in, L.d_out, L.r_live, L.acc_kind, cd)) return SOW_ERR_UNSUPPORTED;
    if (!L.A || !L.B || !L.acc_down || (bwd ? (!L.dy || !L.dx) : (!L.x || !L.y))) return SOW_ERR_NULL;
    if (!al16p(L.A) || !al16p(L.B) || !al16p(L.acc_down)) return SOW_ERR_UNSUPPORTED;
    if (bwd ? (!al16p(L.dy) || !al16p(L.dx)) : (!al16p(L.x) || !al16p(L.y) || !al16p(L.bias) || !al16p(L.h_save))) return SOW_ERR_UNSUPPORTED;
    const size_t need = bwd ? sow_short_workspace_bytes(L.T, L.d_in, L.d_out, L.r_live, L.acc_kind, cd)
                            : sow_forward_short_workspace_bytes(L.T, L.d_in, L.d_out, L.r_live, L.acc_kind, cd);
    if (!L.workspace || L.workspace_bytes < need) return SOW_ERR_WORKSPACE;
    char* ws = ws_base(L.workspace);
    const int K = bwd ? L.d_out : L.d_in, N = bwd ? L.d_in : L.d_out;
    const ShortWs w = short_ws(L.T, K, N, bwd);
    // the data phase keeps dh where the weight phases read it and its partials behind the plan they use
    const WsPlan p = plan_of(L, cd);
    char* part = bwd ? ws + p.total : ws;
    char* hout = bwd ? ws + p.off_dh : (char*)L.h_save;
    const size_t es = esize(cd);
    for (int64_t t0 = 0; t0 < L.T; t0 += 64) {
      SkLayer E{};
      E.x = (const char*)(bwd ? L.dy : L.x) + (size_t)t0 * K * es;
      E.y = (char*)(bwd ? L.dx : L.y) + (size_t)t0 * N * es;
      E.W = L.acc_down, E.A = bwd ? L.B : L.A, E.B = bwd ? L.A : L.B, E.bias = bwd ? nullptr : L.bias;
      E.Py = (float*)part + (size_t)w.S * t0 * N, E.Ph = (float*)(part + w.off_ph) + (size_t)w.S * t0 * 64;
      E.T = (int)(L.T - t0 < 64 ? L.T - t0 : 64), E.d_in = K, E.d_out = N, E.r = L.r_live, E.scale = L.scale;
      E.S = w.S, E.KS = w.KS, E.ncr = w.ncr;
      E.hout = hout ? hout + (size_t)t0 * 64 * es : nullptr;
      e.push_back(E);
    }
  }
  return launch_skinny_short(e.data(), (int)e.size(), cd, bwd, (hipStream_t)stream);
}
int sow_forward_short(const sow_layer_args* layers, int n, int dtype, void* stream) { return short_impl(layers, n, dtype, stream, false); }
int sow_backward_short(const sow_layer_args* layers, int n, int dtype, void* stream) { return short_impl(layers, n, dtype, stream, true); }

// ---- the same on E4M3 / MXFP4 codes read in place (acc_down = the codes, acc_up = the scales; no image, no arena) ----------------
// Entry points and queries of their own: the four above keep refusing the code kinds and answering 0 for them.  The admitted set:
// SOW_ACC_DENSE_FP8 / _FP4 only, one kind per call, bf16 / f16 without flags, 1 <= T <= SOW_SHORT_ROWS_MAX, r_live <= 64, the widths
// of the format (E4M3 8 / 8, MXFP4 d_in % 32 and d_out % 8).
static bool short_codes_shape_ok(int64_t T, int d_in, int d_out, int r_live, int acc_kind, int dtype) {
  return acc_is_codes(acc_kind) && short_shape_ok(T, d_in, d_out, r_live, SOW_ACC_DENSE, dtype) && (acc_kind != SOW_ACC_DENSE_FP4 || d_in % 32 == 0);
}
// the forward's partials take the plan of the 128-column code forms; the data gradient keeps the plain geometry (short_ws)
static ShortWs short_codes_fwd_ws(int64_t T, int d_in, int d_out) {
  ShortWs w;
  short_codes_plan(T, d_in, d_out, &w.S, &w.KS, &w.ncr);
  w.off_ph = al256(skinny_py_bytes(T, d_out, w.S));
  w.bytes = w.off_ph + al256(skinny_ph_bytes(T, w.S));
  return w;
}
size_t sow_forward_short_codes_workspace_bytes(int64_t T, int d_in, int d_out, int r_live, int acc_kind, int dtype) {
  const Dtype f = decode_dtype(dtype);
  if (!short_dtype_ok(f) || !short_codes_shape_ok(T, d_in, d_out, r_live, acc_kind, f.cd)) return 0;
  return 256 + short_codes_fwd_ws(T, d_in, d_out).bytes;
}
// the plan of sow_workspace_bytes(..., SOW_ACC_DENSE, ...) -- the kind the weight phases are called with -- then the larger direction's partials
size_t sow_short_codes_workspace_bytes(int64_t T, int d_in, int d_out, int r_live, int acc_kind, int dtype) {
  const Dtype f = decode_dtype(dtype);
  if (!short_dtype_ok(f) || !short_codes_shape_ok(T, d_in, d_out, r_live, acc_kind, f.cd)) return 0;
  const size_t fw = short_codes_fwd_ws(T, d_in, d_out).bytes, bw = short_ws(T, d_out, d_in, true).bytes;
  return plan_ws(T, d_in, d_out, r_live, 0, SOW_ACC_DENSE, f.cd).total + (fw > bw ? fw : bw) + 256;
}

// The checks and refusal codes of short_impl, every layer before the first launch or dereference.
static int short_codes_impl(const sow_layer_args* layers, int n, int dtype, void* stream, bool bwd) {
  const Dtype f = decode_dtype(dtype);
  const int cd = f.cd;
  if (!f.layer_ok() || cd == SOW_F32) return SOW_ERR_DTYPE;
  if (f.param_f32 || f.native_bit || sw_on(SW_NO_SKINNY)) return SOW_ERR_UNSUPPORTED;
  if (n < 0) return SOW_ERR_SHAPE;
  if (n == 0) return SOW_OK;
  if (!layers) return SOW_ERR_NULL;
  if (n > SK_MAXL) return SOW_ERR_UNSUPPORTED;
  const int kind = layers[0].acc_kind;   // one kind per call: the kernels are instantiated per kind
  for (int i = 0; i < n; ++i) {
    if (!acc_kind_known(layers[i].acc_kind)) return SOW_ERR_SHAPE;
    if (!acc_is_codes(layers[i].acc_kind) || layers[i].acc_kind != kind) return SOW_ERR_UNSUPPORTED;
  }
  const bool fp4 = kind == SOW_ACC_DENSE_FP4;
  std::vector<SkLayer> e;
  for (int i = 0; i < n; ++i) {
    const sow_layer_args& L = layers[i];
    if (L.T < 0 || L.d_in <= 0 || L.d_out <= 0 || L.r_live <= 0) return SOW_ERR_SHAPE;
    if (L.T == 0) continue;
    if (!short_codes_shape_ok(L.T, L.d_in, L.d_out, L.r_live, kind, cd)) return SOW_ERR_UNSUPPORTED;
    if (!L.A || !L.B || !L.acc_down || !L.acc_up || (bwd ? (!L.dy || !L.dx) : (!L.x || !L.y))) return SOW_ERR_NULL;
    if (!al16p(L.A) || !al16p(L.B) || (!fp4 && !al16p(L.acc_down))) return SOW_ERR_UNSUPPORTED;
    // codes and scales are read in 8-byte pieces: MXFP4 as in sow_forward_skinny; the data gradient reads the E4M3 exponents so too
    if (((fp4 ? reinterpret_cast<uintptr_t>(L.acc_down) : 0) | reinterpret_cast<uintptr_t>(L.acc_up)) & 7) return SOW_ERR_UNSUPPORTED;
    if (bwd ? (!al16p(L.dy) || !al16p(L.dx)) : (!al16p(L.x) || !al16p(L.y) || !al16p(L.bias) || !al16p(L.h_save))) return SOW_ERR_UNSUPPORTED;
    const size_t need = bwd ? sow_short_codes_workspace_bytes(L.T, L.d_in, L.d_out, L.r_live, kind, cd)
                            : sow_forward_short_codes_workspace_bytes(L.T, L.d_in, L.d_out, L.r_live, kind, cd);
    if (!L.workspace || L.workspace_bytes < need) return SOW_ERR_WORKSPACE;
    char* ws = ws_base(L.workspace);
    const int K = bwd ? L.d_out : L.d_in, N = bwd ? L.d_in : L.d_out;
    const ShortWs w = bwd ? short_ws(L.T, K, N, true) : short_codes_fwd_ws(L.T, K, N);
    // dh where the weight phases (called with SOW_ACC_DENSE) read it, the partials behind the plan they use
    const WsPlan p = plan_ws(L.T, L.d_in, L.d_out, L.r_live, 0, SOW_ACC_DENSE, cd);
    char* part = bwd ? ws + p.total : ws;
    char* hout = bwd ? ws + p.off_dh : (char*)L.h_save;
    const size_t es = esize(cd);
    for (int64_t t0 = 0; t0 < L.T; t0 += 64) {
      SkLayer E{};
      E.x = (const char*)(bwd ? L.dy : L.x) + (size_t)t0 * K * es;
      E.y = (char*)(bwd ? L.dx : L.y) + (size_t)t0 * N * es;
      E.W = L.acc_down, E.wexp = (const int8_t*)L.acc_up;
      E.A = bwd ? L.B : L.A, E.B = bwd ? L.A : L.B, E.bias = bwd ? nullptr : L.bias;
      E.Py = (float*)part + (size_t)w.S * t0 * N, E.Ph = (float*)(part + w.off_ph) + (size_t)w.S * t0 * 64;
      E.T = (int)(L.T - t0 < 64 ? L.T - t0 : 64), E.d_in = K, E.d_out = N, E.r = L.r_live, E.scale = L.scale;
      E.S = w.S, E.KS = w.KS, E.ncr = w.ncr;
      E.hout = hout ? hout + (size_t)t0 * 64 * es : nullptr;
      e.push_back(E);
    }
  }
  return launch_skinny_short(e.data(), (int)e.size(), cd, bwd, (hipStream_t)stream, kind);
}
int sow_forward_short_codes(const sow_layer_args* layers, int n, int dtype, void* stream) { return short_codes_impl(layers, n, dtype, stream, false); }
int sow_backward_short_codes(const sow_layer_args* layers, int n, int dtype, void* stream) { return short_codes_impl(layers, n, dtype, stream, true); }

static int backward_group_impl(const sow_layer_args* layers, int n, int dtype, int gdt, int phases, int perm, hipStream_t stream) {
  const Phases ph = decode_phases(phases);
  if (!ph.data && !ph.weights()) return SOW_ERR_SHAPE;
  if (!ok_dtype(dtype)) return SOW_ERR_DTYPE;
  if (n < 0) return SOW_ERR_SHAPE;
  if (n == 0) return SOW_OK;
  if (!layers) return SOW_ERR_NULL;
  int rc;
  for (int i = 0; i < n; ++i)
    if ((rc = check_layer(layers[i], true, false))) return rc;
  if (ph.data) {
    ChainParams batch[C2_MAXG];
    ProjGemm gbatch[4];
    int nb = 0, ng = 0;
    for (int i = 0; i < n; ++i) {
      const sow_layer_args& L = layers[i];
      if (L.T == 0) {   // empty batch: everything at once
        if ((rc = backward_impl(L, dtype, gdt, SOW_BWD_DATA | (phases & ~SOW_BWD_DATA), perm, stream))) return rc;
        continue;
      }
      const WsPlan w = plan_of(L, dtype);
      if (L.workspace_bytes < w.total + 255) return SOW_ERR_WORKSPACE;
      if (group_chain_params(L, true, dtype, w, &batch[nb])) {
        if (++nb == C2_MAXG) {
          if ((rc = launch_chain2_group(batch, nb, true, dtype, stream))) return rc;
          nb = 0;
        }
        continue;
      }
      if (L.acc_kind == SOW_ACC_DENSE && L.r_live <= 64) {
        const ProjGemm g = dense_args(dir_view(L, true, ws_base(L.workspace) + w.off_dh));
        if (gemm4h_supported(g, true, dtype)) {
          if ((rc = launch_gemm4h(g, true, dtype, stream))) return rc;
          continue;
        }
        if (!sw_on(SW_NO_GROUPED) && gemm2h_supported(g, true, dtype)) {
          gbatch[ng] = g;
          if (++ng == 4) {
            if ((rc = launch_gemm2h_group(gbatch, ng, true, stream))) return rc;
            ng = 0;
          }
          continue;
        }
      }
      if ((rc = backward_impl(L, dtype, gdt, SOW_BWD_DATA, perm, stream))) return rc;
    }
    if (ng && (rc = launch_gemm2h_group(gbatch, ng, true, stream))) return rc;
    if (nb && (rc = launch_chain2_group(batch, nb, true, dtype, stream))) return rc;
  }
  int rns[TNR_MAXI], rslab[TNR_MAXI];
  const bool rows = group_rows(layers, n, dtype, phases, rns, rslab);
  if (ph.partial && rows) {
    TnRowsItem items[TNR_MAXI];
    for (int i = 0; i < n; ++i) {
      const sow_layer_args& L = layers[i];
      const TnParams tp = tn_params(L, plan_of(L, dtype), ws_base(L.workspace), dtype);
      for (int j = 0; j < 2; ++j) items[2 * i + j] = tn_rows_item(tp.job[j], L.T, rns[2 * i + j], rslab[2 * i + j]);
    }
    if ((rc = launch_tn_rows(items, 2 * n, dtype, stream))) return rc;
  } else if (ph.partial) {
    TnParams batch[TN_MAXG];
    int nb = 0;
    for (int i = 0; i < n; ++i) {
      const sow_layer_args& L = layers[i];
      if (L.T == 0) {
        if (!ph.data && (rc = backward_impl(L, dtype, gdt, phases, perm, stream))) return rc;
        continue;
      }
      const WsPlan w = plan_of(L, dtype);
      if (L.workspace_bytes < w.total + 255) return SOW_ERR_WORKSPACE;
      // the layers of the wide 16-bit kernel share its grouped launch; every other pick runs on its own
      if (!sw_on(SW_NO_GROUPED) && pick_layer_tn(L, w, dtype, &batch[nb]) == TN_DMA_WIDE) {
        if (++nb == TN_MAXG) {
          if ((rc = launch_tn_group(batch, nb, dtype, stream))) return rc;
          nb = 0;
        }
      } else if ((rc = backward_impl(L, dtype, gdt, SOW_BWD_WEIGHTS_PARTIAL, perm, stream)))
        return rc;
    }
    if (nb && (rc = launch_tn_group(batch, nb, dtype, stream))) return rc;
  }
  if (ph.reduce && rows) {
    for (int i = 0; i < n; ++i) {
      const sow_layer_args& L = layers[i];
      ReduceParams rp = make_reduce_params(plan_of(L, dtype), ws_base(L.workspace), L.dA, L.dB, L.dbias, L.d_in, L.d_out, L.r_live,
                                           L.grad_beta);
      rp.job[0].ns = rns[2 * i], rp.job[1].ns = rns[2 * i + 1];
      if ((rc = launch_tn_reduce(rp, gdt, stream))) return rc;
    }
  } else if (ph.reduce) {
    for (int i = 0; i < n; ++i)
      if (layers[i].T != 0 && (rc = backward_impl(layers[i], dtype, gdt, SOW_BWD_WEIGHTS_REDUCE, perm, stream))) return rc;
  }
  return SOW_OK;
}

int sow_backward_group(const sow_layer_args* layers, int n, int dtype, int phases, void* stream_) {
  if (any_codes_acc(layers, n)) return SOW_ERR_UNSUPPORTED;
  hipStream_t stream = (hipStream_t)stream_;
  const Dtype f = decode_dtype(dtype);
  if (f.native_bit && !f.layer_ok()) return SOW_ERR_DTYPE;
  if (!f.param_f32) return backward_group_impl(layers, n, f.cd, f.cd, phases, f.perm(), stream);
  if (!f.layer_ok()) return SOW_ERR_DTYPE;
  if (n <= 0 || !layers || !(phases & SOW_BWD_DATA)) return backward_group_impl(layers, n, f.cd, SOW_F32, phases, 0, stream);
  std::vector<sow_layer_args> packed;
  const int rc = pack_group(layers, n, f.cd, true, f.native, packed, stream);
  return rc ? rc : backward_group_impl(packed.data(), n, f.cd, SOW_F32, phases, 0, stream);
}

// ---- shared-input entry points (chain2_shared.hip) -----------------------------------------------------------------
// Sibling layers on one x: the forward reads x once, the data gradient writes ONE dX.  Admitted: a set that
// group_chain_params takes layer by layer (bf16 / f16, no accumulator, r_live <= 64, T > 8192, chain2 alignment) with one x
// pointer and one d_in; anything else returns SOW_ERR_UNSUPPORTED before anything is launched.  SOW_PARAM_F32 is not
// admitted either, but only after the checks before it: a flagged fp32 dtype gets that far too.
// The data gradient also admits, under SOW_FUSE_ACC, siblings that ALL carry a low-rank accumulator (shared_fused_acc_data,
// chain_shared_acc.hip); the forward does not: a side-by-side phase 1 over the siblings' columns has no room in the registers.
static int shared_common(const sow_layer_args* layers, int n, bool bwd) {
  if (n <= 0) return SOW_ERR_SHAPE;
  if (!layers) return SOW_ERR_NULL;
  for (int i = 0; i < n; ++i) {
    const sow_layer_args& L = layers[i];
    if (L.x != layers[0].x || L.T != layers[0].T || L.d_in != layers[0].d_in) return SOW_ERR_SHAPE;
    if (bwd && L.dx && L.dx != layers[0].dx) return SOW_ERR_SHAPE;
  }
  return SOW_OK;
}
static void shared_fill_dx(const sow_layer_args* layers, int n, sow_layer_args* out) {
  for (int i = 0; i < n; ++i) out[i] = layers[i], out[i].dx = layers[0].dx;   // check_layer wants every dx
}

int sow_forward_shared(const sow_layer_args* layers, int n, int dtype, void* stream) {
  if (any_codes_acc(layers, n)) return SOW_ERR_UNSUPPORTED;
  const Dtype f = decode_dtype(dtype);
  if (!ok_dtype(f.cd)) return SOW_ERR_DTYPE;
  int rc;
  if ((rc = shared_common(layers, n, false))) return rc;
  for (int i = 0; i < n; ++i)
    if ((rc = check_layer(layers[i], false, false))) return rc;
  if (sw_on(SW_NO_SHARED_X) || f.param_f32 || f.native_bit || n > C2_MAXG || layers[0].T == 0) return SOW_ERR_UNSUPPORTED;
  ChainParams ps[C2_MAXG];
  for (int i = 0; i < n; ++i)
    if (!group_chain_params(layers[i], false, f.cd, WsPlan{}, &ps[i])) return SOW_ERR_UNSUPPORTED;
  return launch_chain2_shared(ps, n, false, f.cd, (hipStream_t)stream);
}

int sow_backward_shared(const sow_layer_args* layers, int n, int dtype, int phases, void* stream_) {
  if (any_codes_acc(layers, n)) return SOW_ERR_UNSUPPORTED;
  hipStream_t stream = (hipStream_t)stream_;
  const Dtype f = decode_dtype(dtype);
  const int cd = f.cd;
  if (!ok_dtype(cd)) return SOW_ERR_DTYPE;
  int rc;
  if ((rc = shared_common(layers, n, true))) return rc;
  if (n > C2_MAXG) return SOW_ERR_UNSUPPORTED;
  if (f.param_f32 || f.native_bit) return SOW_ERR_UNSUPPORTED;   // (SOW_ACC_NATIVE: the code of SOW_PARAM_F32)
  sow_layer_args filled[C2_MAXG];
  shared_fill_dx(layers, n, filled);
  if (!(phases & SOW_BWD_DATA)) return backward_group_impl(filled, n, cd, cd, phases, 0, stream);
  for (int i = 0; i < n; ++i)
    if ((rc = check_layer(filled[i], true, false))) return rc;
  if (sw_on(SW_NO_SHARED_X) || filled[0].T == 0) return SOW_ERR_UNSUPPORTED;
  ChainParams ps[C2_MAXG];
  bool streaming = true;
  for (int i = 0; i < n; ++i) {
    const sow_layer_args& L = filled[i];
    const WsPlan w = plan_of(L, cd);
    if (!group_chain_params(L, true, cd, w, &ps[i])) {
      // not the streaming set: siblings that all carry a low-rank accumulator, under SOW_FUSE_ACC, or nothing
      if ((rc = shared_fused_acc_data(filled, n, f, stream))) return rc;
      streaming = false;
      break;
    }
    if (L.workspace_bytes < w.total + 255) return SOW_ERR_WORKSPACE;
    ps[i].beta = filled[0].grad_beta;   // dX = grad_beta * dX + sum_i dh_i A_i^T
  }
  if (streaming && (rc = launch_chain2_shared(ps, n, true, cd, stream))) return rc;
  // the weight phases read each layer's dh where the grouped data phase leaves it: exactly sow_backward_group's code
  const int wph = phases & ~SOW_BWD_DATA;
  return decode_phases(wph).weights() ? backward_group_impl(filled, n, cd, cd, wph, 0, stream) : SOW_OK;
}

// the group entry points' checks for the two plan queries below
static int check_group(const sow_layer_args* layers, int n) {
  for (int i = 0; i < n; ++i) {
    const int rc = check_layer(layers[i], true, false);
    if (rc) return rc;
  }
  return SOW_OK;
}

int sow_backward_group_plan(const sow_layer_args* layers, int n, int dtype, int phases, int* slabs_out) {
  if (any_codes_acc(layers, n)) return SOW_ERR_UNSUPPORTED;
  const Dtype f = decode_dtype(dtype);   // the plan does not depend on the parameter dtype
  if (!f.layer_ok()) return SOW_ERR_DTYPE;
  if (n < 0) return SOW_ERR_SHAPE;
  if (n == 0) return 0;
  if (!layers) return SOW_ERR_NULL;
  int rc;
  if ((rc = check_group(layers, n))) return rc;
  int rns[TNR_MAXI], rslab[TNR_MAXI];
  const bool rows = group_rows(layers, n, f.cd, phases, rns, rslab);
  if (slabs_out)
    for (int i = 0; i < n; ++i) {
      const sow_layer_args& L = layers[i];
      const int ns = L.T > 0 && L.r_live <= 64 ? plan_of(L, f.cd).ns : 0;
      slabs_out[2 * i] = rows ? rns[2 * i] : ns;
      slabs_out[2 * i + 1] = rows ? rns[2 * i + 1] : ns;
    }
  return rows ? 1 : 0;
}

// Debug export (declared by tests/test_host_tn_pick_cpu.py only): the weight-gradient kernel of n <= TN_MAXG layers [T, d_in[i]]
// x [T, d_out[i]] of rank r_live without accumulator, as sow_backward_ex (n = 1) or sow_backward_group (n > 1) with `phases`
// would choose it.  Nothing is launched or dereferenced: the operands are fake pointers through the real plan_ws / tn_params /
// group_rows path, 16-byte aligned except where `misalign` says one element further (bit 0 x, 1 dY, 2 h_save, 3 workspace).
// out[9 i ..]: TnKernel, blocks of work (tn_blocks), ns and slab_len of x's operand, of dY's operand, bytes of the two partial
// regions of the plan (wide rank: of its one region, and 0), 1 when the layer shares a grouped launch.
int sow_debug_tn_pick(int n, int64_t T, const int* d_in, const int* d_out, int r_live, int has_dbias, int dtype, int phases,
                      int misalign, int64_t* out) {
  if (n < 1 || n > TN_MAXG || T < 0 || !d_in || !d_out || !out || !ok_dtype(dtype)) return SOW_ERR_SHAPE;
  auto fake = [&](int bit) { return (void*)(((uintptr_t)1 << 20) + ((misalign >> bit) & 1) * esize(dtype)); };
  sow_layer_args Ls[TN_MAXG];
  for (int i = 0; i < n; ++i) {
    const size_t bytes = plan_ws(T, d_in[i], d_out[i], r_live, 0, SOW_ACC_NONE, dtype).total + 512;
    Ls[i] = single_layer(fake(0), fake(4), fake(4), nullptr, nullptr, nullptr, nullptr, fake(2), fake(1), fake(4), fake(4), fake(4),
                         has_dbias ? fake(4) : nullptr, T, d_in[i], d_out[i], r_live, 0, SOW_ACC_NONE, 1.f, 0.f, fake(3), bytes);
  }
  int rns[TNR_MAXI], rslab[TNR_MAXI];
  const bool rows = n > 1 && T > 0 && group_rows(Ls, n, dtype, phases, rns, rslab);
  for (int i = 0; i < n; ++i) {
    const sow_layer_args& L = Ls[i];
    const WsPlan w = plan_of(L, dtype);
    int64_t* o = out + 9 * i;
    for (int j = 0; j < 9; ++j) o[j] = 0;
    if (T == 0) continue;   // TN_NONE: the gradients are zeroed, no kernel of the family runs
    TnParams tp{};
    const TnKernel k = rows ? TN_ROWS : pick_layer_tn(L, w, dtype, &tp);
    o[0] = k, o[8] = rows || (n > 1 && k == TN_DMA_WIDE && !sw_on(SW_NO_GROUPED));
    if (L.r_live > 64) {
      int len = 0;
      const int ns = k == TN_WIDE_RANK ? tnw_pick_slabs(T, L.d_in, L.d_out, &len) : 0;
      o[1] = (int64_t)ns * ((L.d_in + 63) / 64 + (L.d_out + 63) / 64), o[2] = o[4] = ns, o[3] = o[5] = len, o[6] = (int64_t)w.pw_bytes;
      continue;
    }
    o[6] = (int64_t)(w.off_p1 - w.off_p0), o[7] = (int64_t)(w.off_planes - w.off_p1);
    if (rows) {
      for (int j = 0; j < 2; ++j) o[2 + 2 * j] = rns[2 * i + j], o[3 + 2 * j] = rslab[2 * i + j];
      o[1] = (int64_t)rns[2 * i] * (((L.d_in + 63) / 64 + 15) / 16) + (int64_t)rns[2 * i + 1] * (((L.d_out + 63) / 64 + 15) / 16);
    } else {
      o[1] = tn_blocks(k, tp), o[2] = o[4] = tp.ns, o[3] = o[5] = tp.slab_len;
    }
  }
  return SOW_OK;
}

int sow_backward_group_reduce_desc(const sow_layer_args* layers, int n, int dtype, int phases, void* descs_out, int* blocks_out) {
  if (any_codes_acc(layers, n)) return SOW_ERR_UNSUPPORTED;
  const Dtype f = decode_dtype(dtype);
  if (!f.layer_ok()) return SOW_ERR_DTYPE;
  if (n < 0) return SOW_ERR_SHAPE;
  if (n == 0) return SOW_OK;
  if (!layers || !descs_out || !blocks_out) return SOW_ERR_NULL;
  int rc;
  if ((rc = check_group(layers, n))) return rc;
  // Not group_rows(): `phases` are the flags of the PARTIAL call, whose reduction is deferred, so the group-planned slab
  // counts apply exactly when that call asked for them (SOW_BWD_GROUP_SLABS), whatever its other phase bits say.
  int rns[TNR_MAXI], rslab[TNR_MAXI];
  const bool rows = (phases & SOW_BWD_GROUP_SLABS) && group_rows_plan(layers, n, f.cd, phases, rns, rslab);
  for (int i = 0; i < n; ++i) {
    const sow_layer_args& L = layers[i];
    char* out = (char*)descs_out + (size_t)i * sizeof(ReduceParams);
    if ((rc = sow_backward_reduce_desc(L.dA, L.dB, L.dbias, L.T, L.d_in, L.d_out, L.r_live, L.r_acc, L.acc_kind, L.grad_beta, f.cd,
                                       L.workspace, L.workspace_bytes, out, blocks_out + i)))
      return rc;
    if (rows) {
      ReduceParams rp;
      memcpy(&rp, out, sizeof rp);
      rp.job[0].ns = rns[2 * i], rp.job[1].ns = rns[2 * i + 1];
      memcpy(out, &rp, sizeof rp);
    }
  }
  return SOW_OK;
}

int sow_gemm(const void* A, int64_t lda, int trans_a, const void* B, int64_t ldb, int trans_b, void* C, int64_t ldc,
             const void* bias, int64_t M, int N, int K, float alpha, float beta, int dtype, void* stream) {
  return sow_gemm_ex(A, lda, trans_a, B, ldb, trans_b, C, ldc, bias, M, N, K, alpha, beta, dtype, nullptr, 0, stream);
}

size_t sow_gemm_workspace_bytes(int64_t M, int N, int K, int trans_a, int dtype) {
  dtype = nofuse(dtype);
  if (trans_a || (dtype != SOW_BF16 && dtype != SOW_F16) || M <= 0 || N <= 0 || K <= 0) return 0;
  return gemm4_splitk_bytes(M, N, K, false);
}

int sow_gemm_ex(const void* A, int64_t lda, int trans_a, const void* B, int64_t ldb, int trans_b, void* C, int64_t ldc,
                const void* bias, int64_t M, int N, int K, float alpha, float beta, int dtype, void* workspace,
                size_t workspace_bytes, void* stream) {
  dtype = nofuse(dtype);
  if (flagged(dtype)) return SOW_ERR_DTYPE;   // SOW_PARAM_F32 is for the layer entry points only
  if (!trans_a)
    return gemm_auto(A, lda, B, ldb, trans_b != 0, C, ldc, bias, M, N, K, alpha, beta, dtype, (hipStream_t)stream, workspace,
                     workspace_bytes);
  return launch_gemm(A, lda, trans_a != 0, B, ldb, trans_b != 0, C, ldc, bias, M, N, K, alpha, beta, dtype, (hipStream_t)stream);
}

// sow_qr_thin factors panels wider than QR_BLOCK_MIN columns by blocks (qr_blocked.hip).  Measured crossover: DESIGN.md
// "Blocked QR"; it must stay >= 64 (the r <= 64 re-initialisation panels keep the one-workgroup kernel).
constexpr int QR_BLOCK_MIN = 64;
constexpr int QR_TAIL_K = 512;   // rows per partial product of the R tail on the blocked route
struct QrPlan {
  int kc;
  size_t off_pt, off_qt, off_w, off_r, total;
  size_t off_t, total_thin;   // sow_qr_thin only: the blocked route's T tiles behind everything else (kc > QR_BLOCK_MIN)
};
static QrPlan plan_qr(int m, int n, int k, int in_dtype, int need_r, int out_dtype_is_f32) {
  QrPlan q{};
  q.kc = k < m ? k : m;
  if (n < q.kc) q.kc = n;
  size_t off = 0;
  q.off_pt = off;
  off += al256((size_t)q.kc * m * 4);
  q.off_qt = off;
  off += al256((size_t)k * m * 4);
  q.off_w = off;
  if (need_r && n > q.kc && in_dtype != SOW_F32) off += al256((size_t)m * (n - q.kc) * 4);
  q.off_r = off;
  if (need_r && n > q.kc && !out_dtype_is_f32) off += al256((size_t)k * (n - q.kc) * 4);
  q.total = off;
  // a pure function of the shape: the T tiles are planned whatever the NO_BLOCKED_QR switch says
  q.off_t = off;
  if (q.kc > QR_BLOCK_MIN) off += al256(qr_blocked_t_floats(q.kc) * 4);
  q.total_thin = off;
  return q;
}

size_t sow_qr_workspace_bytes(int m, int n, int k, int in_dtype, int need_r) {
  in_dtype = nofuse(in_dtype);
  if (m <= 0 || n <= 0 || k <= 0) return 0;
  return plan_qr(m, n, k, in_dtype, need_r, 0).total_thin + 256;
}

int sow_qr_thin(const void* W, int64_t ldw, int m, int n, int in_dtype, int k, void* Q_out, int64_t ldq, void* R_out,
                int64_t ldr, int out_dtype, void* workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  in_dtype = nofuse(in_dtype), out_dtype = nofuse(out_dtype);
  if (!ok_dtype(in_dtype) || !ok_dtype(out_dtype)) return SOW_ERR_DTYPE;   // rejects SOW_PARAM_F32 as well
  if (m <= 0 || n <= 0 || k <= 0 || k > m) return SOW_ERR_SHAPE;
  if (!W || !Q_out || !workspace) return SOW_ERR_NULL;
  const QrPlan q = plan_qr(m, n, k, in_dtype, R_out != nullptr, out_dtype == SOW_F32);
  if (workspace_bytes < q.total_thin + 255) return SOW_ERR_WORKSPACE;
  char* ws = ws_base(workspace);
  float* Pt = (float*)(ws + q.off_pt);
  float* Qt = (float*)(ws + q.off_qt);
  int rc;
  const bool blocked = q.kc > QR_BLOCK_MIN && !sw_on(SW_NO_BLOCKED_QR);
  if (blocked)
    rc = launch_qr_blocked(W, ldw, in_dtype, m, q.kc, k, Pt, Qt, (float*)(ws + q.off_t), stream);
  else
    rc = launch_qr_panel(W, ldw, in_dtype, m, q.kc, k, Pt, Qt, stream);
  if (rc) return rc;
  rc = launch_qr_copy_out(Qt, Pt, Q_out, ldq, R_out, ldr, out_dtype, m, q.kc, k, k, stream);
  if (rc) return rc;
  if (R_out && n > q.kc) {
    // R[:k, kc:] = Q[:, :k]^T W[:, kc:]   (fp32 GEMM: A = Qt stored [k, m], B = W columns kc.., k-major)
    const int nt = n - q.kc;
    const void* Bp;
    int64_t ldb;
    if (in_dtype == SOW_F32) {
      Bp = (const float*)W + q.kc, ldb = ldw;
    } else {
      float* wf = (float*)(ws + q.off_w);
      rc = launch_cast_copy((const char*)W + q.kc * esize(in_dtype), ldw, in_dtype, wf, nt, SOW_F32, m, nt, stream);
      if (rc) return rc;
      Bp = wf, ldb = nt;
    }
    // The blocked route sums over the rows in chunks of QR_TAIL_K (C += partial product, rounded once per chunk); the
    // one-workgroup route keeps its single product (the same bits as before).  Measured where it matters: 2048 x 5461 bf16,
    // k = 2048 (tests/test_gpu_step_elementwise.py::test_qr_thin_large_k).  Its tail has 3413 columns, an odd row pitch, so
    // every chunk runs gemm_kernel<float> on the exact fp32 MFMA whatever F32_EXACT says (the 3 x bf16 split needs
    // vector-aligned rows), and 2048 = 4 x 512 has no ragged last chunk.  Worst |error| / limit of the tail check, always
    // at element (202, 2290), error of one sign: 0.94 as one product from the one-workgroup Q, 1.03 as one product from
    // the blocked Q, 0.31 in four chunks (profiles/qr_blocked.txt).  A last chunk shorter than 16 rows or not a multiple
    // of 4 may take the exact kernel while the others take the split; both are fp32 products of the same contract.
    const int kstep = blocked ? QR_TAIL_K : m;
    float* rt = out_dtype == SOW_F32 ? (float*)R_out + q.kc : (float*)(ws + q.off_r);
    const int64_t ldt = out_dtype == SOW_F32 ? ldr : nt;
    for (int k0 = 0; k0 < m; k0 += kstep) {
      const int kk = m - k0 < kstep ? m - k0 : kstep;
      rc = launch_gemm(Qt + k0, m, false, (const float*)Bp + (int64_t)k0 * ldb, ldb, false, rt, ldt, nullptr, k, nt, kk, 1.f,
                       k0 ? 1.f : 0.f, SOW_F32, stream);
      if (rc) return rc;
    }
    if (out_dtype != SOW_F32) {
      rc = launch_cast_copy(rt, nt, SOW_F32, (char*)R_out + q.kc * esize(out_dtype), ldr, out_dtype, k, nt, stream);
      if (rc) return rc;
    }
  }
  return SOW_OK;
}

int sow_accumulate_batch(const sow_accumulate_args* items, int n, int dtype, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  dtype = nofuse(dtype);
  if (!ok_dtype(dtype)) return SOW_ERR_DTYPE;
  if (n < 0) return SOW_ERR_SHAPE;
  if (n == 0) return SOW_OK;
  if (!items) return SOW_ERR_NULL;
  std::vector<AccItem> its((size_t)n);
  std::vector<void*> zp;
  std::vector<int64_t> zb;
  for (int i = 0; i < n; ++i) {
    const sow_accumulate_args& a = items[i];
    if (a.d_in <= 0 || a.d_out <= 0 || a.r <= 0 || a.r > 64) return SOW_ERR_SHAPE;
    if (!a.acc || !a.A || !a.B) return SOW_ERR_NULL;
    AccItem& t = its[(size_t)i];
    t.acc = a.acc, t.A = a.A, t.B = a.B, t.draw = a.draw, t.A_new = a.A_new, t.ld_draw = a.ld_draw;
    t.d_in = a.d_in, t.d_out = a.d_out, t.r = a.r, t.r_new = a.r_new, t.scale = a.scale, t.beta = a.acc_beta;
    t.Pt = t.Qt = nullptr, t.kc = 0;
    if (a.draw) {
      if (!a.A_new || !a.workspace || a.r_new <= 0 || a.r_new > a.d_in || a.draw_cols <= 0 || a.ld_draw < a.draw_cols)
        return a.A_new && a.workspace ? SOW_ERR_SHAPE : SOW_ERR_NULL;
      const QrPlan q = plan_qr(a.d_in, a.draw_cols, a.r_new, dtype, 0, 0);
      if (a.workspace_bytes < q.total + 255) return SOW_ERR_WORKSPACE;
      char* ws = ws_base(a.workspace);
      t.kc = q.kc, t.Pt = (float*)(ws + q.off_pt), t.Qt = (float*)(ws + q.off_qt);
    }
    if (a.zero && a.zero_bytes > 0) zp.push_back(a.zero), zb.push_back(a.zero_bytes);
  }
  int rc = launch_accumulate_batch(its.data(), n, dtype, stream);
  if (rc) return rc;
  return zp.empty() ? SOW_OK : launch_multi_zero(zp.data(), zb.data(), (int)zp.size(), stream);
}

int sow_zero_state(void* const* ptrs, const int64_t* bytes, int n, void* stream) {
  if (n < 0) return SOW_ERR_SHAPE;
  if (n == 0) return SOW_OK;
  if (!ptrs || !bytes) return SOW_ERR_NULL;
  return launch_multi_zero(ptrs, bytes, n, (hipStream_t)stream);
}

int sow_adamw_flat(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, int64_t n, float lr, double beta1,
                   double beta2, float eps, float weight_decay, int step, float grad_scale, int dtype, int state_dtype,
                   void* stream) {
  dtype = nofuse(dtype), state_dtype = nofuse(state_dtype);
  if (flagged(dtype) || flagged(state_dtype)) return SOW_ERR_DTYPE;
  if (step < 1) return SOW_ERR_SHAPE;
  return launch_adamw_flat(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale,
                           dtype, state_dtype, (hipStream_t)stream);
}

int sow_adamw_flat_seg(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, const sow_adamw_segment* segs,
                       int n_segs, double beta1, double beta2, float eps, float grad_scale, int dtype, int state_dtype,
                       void* stream) {
  dtype = nofuse(dtype), state_dtype = nofuse(state_dtype);
  if (flagged(dtype) || flagged(state_dtype)) return SOW_ERR_DTYPE;
  return launch_adamw_flat_seg(param, grad, exp_avg, exp_avg_sq, segs, n_segs, beta1, beta2, eps, grad_scale, dtype,
                               state_dtype, (hipStream_t)stream);
}

size_t sow_grad_stats_workspace_bytes(int64_t n) { return grad_stats_workspace_bytes(n); }

int sow_grad_stats_flat(const void* grad, int64_t n, int dtype, float grad_scale, float max_norm, const double* extra_sumsq,
                        const float* loss_scale, const float* extra_found_inf, int32_t* skip_counters, int n_counters,
                        void* workspace, size_t workspace_bytes, sow_grad_stats* out, void* stream) {
  dtype = nofuse(dtype);
  if (flagged(dtype)) return SOW_ERR_DTYPE;
  return launch_grad_stats(grad, n, dtype, grad_scale, max_norm, extra_sumsq, loss_scale, extra_found_inf, skip_counters,
                           n_counters, workspace, workspace_bytes, out, (hipStream_t)stream);
}

int sow_adamw_flat_seg_stats(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, const sow_adamw_segment* segs,
                             const int* seg_counter, int n_segs, double beta1, double beta2, float eps,
                             const sow_grad_stats* stats, int skip_nonfinite, const int32_t* skip_counters, int n_counters,
                             int dtype, int state_dtype, void* stream) {
  dtype = nofuse(dtype), state_dtype = nofuse(state_dtype);
  if (flagged(dtype) || flagged(state_dtype)) return SOW_ERR_DTYPE;
  return launch_adamw_flat_seg_stats(param, grad, exp_avg, exp_avg_sq, segs, seg_counter, n_segs, beta1, beta2, eps, stats,
                                     skip_nonfinite, skip_counters, n_counters, dtype, state_dtype, (hipStream_t)stream);
}

int sow_ttadam_dense(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, double beta1,
                     double beta2, float eps, float step_size, float lr_times_wd, int clamp_v, void* stream) {
  return launch_ttadam_dense(param, grad, exp_avg, exp_avg_sq, n, beta1, beta2, eps, step_size, lr_times_wd, clamp_v,
                             (hipStream_t)stream);
}

int sow_tt_kron_core(const float* A, const float* B, float* out, int ra0, int rb0, int ij, int ra1, int rb1,
                     void* stream) {
  return launch_tt_kron_core(A, B, out, ra0, rb0, ij, ra1, rb1, (hipStream_t)stream);
}

int sow_absmax(const float* x, int64_t n, float* out, void* stream) {
  return launch_absmax(x, n, out, (hipStream_t)stream);
}

int sow_small_inverse(const float* A, float* out, int batch, int r, void* stream) {
  return launch_small_inverse(A, out, batch, r, (hipStream_t)stream);
}

int sow_axpby(const void* x, void* y, int64_t n, float a, float b, int dtype, void* stream) {
  dtype = nofuse(dtype);
  if (flagged(dtype)) return SOW_ERR_DTYPE;
  return launch_axpby(x, y, n, a, b, dtype, (hipStream_t)stream);
}

int sow_acc_dequantize(const void* q, const void* exps, int d_in, int d_out, void* dst, int64_t ldd, int dst_dtype,
                       void* stream) {
  if (d_in < 0 || d_out < 0 || ldd < d_out) return SOW_ERR_SHAPE;
  if (dst_dtype != SOW_BF16 && dst_dtype != SOW_F16) return SOW_ERR_DTYPE;
  if (d_in == 0 || d_out == 0) return SOW_OK;
  if (!q || !exps || !dst) return SOW_ERR_NULL;
  if (d_out % 8 || ldd % 8) return SOW_ERR_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(exps)) & 7 || !al16p(dst)) return SOW_ERR_ALIGN;
  return launch_acc_dequantize(q, exps, d_in, d_out, dst, ldd, dst_dtype, (hipStream_t)stream);
}

int sow_acc_dequantize_fp4(const void* codes, const void* scales, int d_in, int d_out, void* dst, int64_t ldd, int dst_dtype,
                           void* stream) {
  if (d_in < 0 || d_out < 0 || ldd < d_out) return SOW_ERR_SHAPE;
  if (dst_dtype != SOW_BF16 && dst_dtype != SOW_F16) return SOW_ERR_DTYPE;
  if (d_in == 0 || d_out == 0) return SOW_OK;
  if (!codes || !scales || !dst) return SOW_ERR_NULL;
  if (d_in % 32 || d_out % 8 || ldd % 8) return SOW_ERR_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(codes) | reinterpret_cast<uintptr_t>(scales)) & 7 || !al16p(dst)) return SOW_ERR_ALIGN;
  return launch_acc_dequantize_fp4(codes, scales, d_in, d_out, dst, ldd, dst_dtype, (hipStream_t)stream);
}

int sow_cast_copy(const void* src, int64_t lds, int src_dtype, void* dst, int64_t ldd, int dst_dtype, int64_t rows,
                  int cols, void* stream) {
  src_dtype = nofuse(src_dtype), dst_dtype = nofuse(dst_dtype);
  if (flagged(src_dtype) || flagged(dst_dtype) || !ok_dtype(src_dtype) || !ok_dtype(dst_dtype)) return SOW_ERR_DTYPE;
  if (!src || !dst) return SOW_ERR_NULL;
  return launch_cast_copy(src, lds, src_dtype, dst, ldd, dst_dtype, rows, cols, (hipStream_t)stream);
}

}  // extern "C"
