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
                                                   "NO_SKINNY",      "NO_FUSED_ACC",   "NO_F16_TN",
                                                   "NO_ROW_ALIGN",   "NO_H_ROWS"};
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
static inline bool al4p(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
static inline bool al16p(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// SOW_PARAM_F32: the compute dtype of a flagged dtype (*pf = flag present); -1 for a combination no layer entry point takes
// SOW_FUSE_ACC is stripped here: the entry points where the permission acts read it with fuse_of() first
static inline int split_dtype(int d, bool* pf) {
  d &= ~SOW_FUSE_ACC;
  *pf = (d & SOW_PARAM_F32) != 0;
  const int cd = d & ~SOW_PARAM_F32;
  if (!ok_dtype(cd) || (*pf && cd == SOW_F32)) return -1;
  return cd;
}
static inline bool flagged(int d) { return (d & SOW_PARAM_F32) != 0; }
// SOW_FUSE_ACC: the permission is ignored together with SOW_PARAM_F32
static inline bool fuse_of(int d) { return (d & SOW_FUSE_ACC) != 0 && !flagged(d); }
static inline int nofuse(int d) { return d & ~SOW_FUSE_ACC; }

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

// row-major A, plain product: the streaming kernel when it fills the chip, else the 128x128 kernel
static int gemm_auto(const void* A, int64_t lda, const void* B, int64_t ldb, bool transB, void* C, int64_t ldc,
                     const void* bias, int64_t M, int N, int K, float alpha, float beta, int dtype, hipStream_t stream,
                     void* ws = nullptr, size_t ws_bytes = 0) {
  if (dtype == SOW_F16) {
    // f16 has gemm4 (and its split-K form) only: taken where its 256 x 256 tiles fill at least half of the chip, as for bf16
    // (launch_gemm2); shorter products and the FORCE_GEMM_V1 / GEMM4 = 0 switches take the generic kernel
    const int g4 = sw(SW_GEMM4);
    const int64_t work = (int64_t)ceil_div(M, 256) * ceil_div(N, 256) * gemm4_splits(M, N, K, false, ws, ws_bytes);
    if (!sw_on(SW_FORCE_GEMM_V1) && (g4 > 0 || (g4 < 0 && work >= 120)) &&
        gemm4_supported(A, lda, B, ldb, transB, nullptr, 0, nullptr, 0, C, ldc, bias, M, N, K, dtype))
      return launch_gemm4(A, lda, B, ldb, transB, nullptr, 0, nullptr, 0, 0, C, ldc, bias, M, N, K, alpha, beta, stream, ws,
                          ws_bytes, dtype);
    return launch_gemm(A, lda, false, B, ldb, transB, C, ldc, bias, M, N, K, alpha, beta, dtype, stream);
  }
  if (gemm2_supported(A, lda, B, ldb, transB, nullptr, 0, nullptr, 0, C, ldc, bias, M, N, K, dtype))
    return launch_gemm2(A, lda, B, ldb, transB, nullptr, 0, nullptr, 0, 0, C, ldc, bias, M, N, K, alpha, beta, stream, ws, ws_bytes);
  return launch_gemm(A, lda, false, B, ldb, transB, C, ldc, bias, M, N, K, alpha, beta, dtype, stream);
}

extern "C" {

int sow_version(void) { return 120; }

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
  int ns, slab_len;
  int ns_cap;   // slabs the partial regions can hold (group-planned slab counts may exceed the single-layer choice)
};
constexpr int64_t C3F_MIN_T = 8192;   // chain3f_supported's threshold
// fuse: the caller's SOW_FUSE_ACC permission.  On an admitted shape the wide region also holds the factors of the fused pass
// (r_acc + r_live columns); such a layer has r_live <= 64, so the region is the plan's last and every other offset is the
// unflagged plan's: a flagged workspace serves the unflagged kernels as it is.  A pure function of its arguments.
static WsPlan plan_ws(int64_t T, int d_in, int d_out, int r_live, int r_acc, int acc_kind, int dtype, bool fuse = false) {
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
    const int cg_in = (d_in + 63) / 64, cg_out = (d_out + 63) / 64;
    const int quads = (dtype == SOW_F32 && tn_f32q_shape_ok(T, d_in, d_out)) ? (cg_in + 3) / 4 + (cg_out + 3) / 4 : 0;
    w.ns = tn_pick_slabs(T, cg_in + cg_out, (cg_in + 1) / 2 + (cg_out + 1) / 2, quads, dtype, &w.slab_len);
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
    w.fused = fuse && acc_kind == SOW_ACC_LOWRANK && fused_acc_shape_ok(r_live, r_acc, d_in, d_out, dtype);
    if (w.fused) {
      const size_t fb = chain_wide_pack_bytes(r_acc + r_live, d_in, d_out);
      if (fb > w.wide_bytes) w.wide_bytes = fb;
    }
    off += al256(w.wide_bytes);
  }
  // token-slab partials of the wide weight-gradient kernel (skinny_tn_wide.hip)
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

// ---- fp32 parameters (SOW_PARAM_F32) ----------------------------------------------------------------------
// The fp32 A, B, bias and accumulator of a call are rounded once to the compute dtype into a region of the layer's workspace
// past the compute-dtype plan (pack_params_kernel, misc.hip); the bf16 / f16 kernels then read the packed copies, in the
// layouts they read from the caller.  Packed again at every call: the factors change at every optimizer step.
static inline size_t pack_elems_bytes(int64_t n) { return al256((size_t)n * 2); }
static size_t pack_bytes(int d_in, int d_out, int r_live, int r_acc, int acc_kind) {
  size_t b = pack_elems_bytes((int64_t)d_in * r_live) + pack_elems_bytes((int64_t)r_live * d_out) + pack_elems_bytes(d_out);
  if (acc_kind == SOW_ACC_DENSE) b += pack_elems_bytes((int64_t)d_in * d_out);
  if (acc_kind == SOW_ACC_LOWRANK) b += pack_elems_bytes((int64_t)d_in * r_acc) + pack_elems_bytes((int64_t)r_acc * d_out);
  return b;
}
// Appends the pack items of layer L (T > 0, pointers checked) to `items` and points L's parameter operands at the packed
// copies.  The packed copies go past the compute-dtype plan (where they never touch what a backward phase leaves in the
// workspace), except for a forward (fwd) whose kernels need no scratch (sow_forward_workspace_bytes = 0 for the compute
// dtype) given a workspace sized by the flagged forward query only: there they start the workspace.  Such a forward then runs
// without workspace, exactly as the unflagged call.
static int pack_layer(sow_layer_args& L, int cd, bool fwd, std::vector<PackItem>& items) {
  const int r_acc = L.acc_kind == SOW_ACC_LOWRANK ? L.r_acc : 0;
  const WsPlan w = plan_ws(L.T, L.d_in, L.d_out, L.r_live, r_acc, L.acc_kind, cd);
  const size_t pack = pack_bytes(L.d_in, L.d_out, L.r_live, r_acc, L.acc_kind);
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
  if (L.acc_kind == SOW_ACC_DENSE) put(L.acc_down, (int64_t)L.d_in * L.d_out);
  if (L.acc_kind == SOW_ACC_LOWRANK) {
    put(L.acc_down, (int64_t)L.d_in * r_acc);
    put(L.acc_up, (int64_t)r_acc * L.d_out);
  }
  return SOW_OK;
}
static sow_layer_args single_layer(const void* A, const void* B, const void* acc_down, const void* acc_up, const void* bias,
                                   int64_t T, int d_in, int d_out, int r_live, int r_acc, int acc_kind, void* workspace,
                                   size_t workspace_bytes) {
  sow_layer_args L{};
  L.A = A, L.B = B, L.acc_down = acc_down, L.acc_up = acc_up, L.bias = bias;
  L.T = T, L.d_in = d_in, L.d_out = d_out, L.r_live = r_live, L.r_acc = r_acc, L.acc_kind = acc_kind;
  L.workspace = workspace, L.workspace_bytes = workspace_bytes;
  return L;
}

// One term of a wide-rank layer on the fused chain (chain_wide.hip), the factors packed into the workspace's wide region;
// SOW_ERR_UNSUPPORTED: nothing launched, the caller composes generic GEMMs.  Forward (bwd = false): F1 = A-like [D1][r],
// F2 = B-like [r][D2]; data gradient: F1 = B-like [r][D1], F2 = A-like [D2][r].
// rag: a term of an admitted ragged layer (rag_layer; the NO_WIDE_CHAIN switch does not apply); any other caller gets
// SOW_ERR_UNSUPPORTED for ragged widths, so that they keep the generic kernels.
static int wide_chain(const void* X, void* Y, const void* F1, int64_t ldf1, const void* F2, int64_t ldf2, void* Hsave,
                      const void* bias, int64_t T, int D1, int D2, int r, float hscale, float yscale, float beta, bool bwd,
                      int dtype, char* ws, const WsPlan& w, size_t workspace_bytes, hipStream_t stream, bool rag = false) {
  const bool ragged = D1 % 8 != 0 || D2 % 8 != 0;
  if ((ragged ? !rag : sw_on(SW_NO_WIDE_CHAIN)) || !ws || !w.wide_bytes || workspace_bytes < w.total + 255 ||
      chain_wide_pack_bytes(r, D1, D2) > w.wide_bytes)
    return SOW_ERR_UNSUPPORTED;
  WideArgs a{};
  a.X = X, a.Y = Y, a.F1 = F1, a.F2 = F2, a.ldf1 = ldf1, a.ldf2 = ldf2, a.Hsave = Hsave, a.bias = bias;
  a.M = T, a.D1 = D1, a.D2 = D2, a.r = r, a.hscale = hscale, a.yscale = yscale, a.beta = beta, a.bwd = bwd ? 1 : 0;
  a.pack = ws + w.off_wide, a.pack_bytes = w.wide_bytes;
  return launch_chain_wide(a, dtype, stream);
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
  bool pf;
  dtype = split_dtype(dtype, &pf);   // the descriptor is the same with fp32 gradients: sow_reduce_batch picks the output type
  if (dtype < 0) return SOW_ERR_DTYPE;
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
  const WsPlan w = plan_ws(T, d_in, d_out, r_live, r_acc, acc_kind, dtype);
  if (workspace_bytes < w.total + 255) return SOW_ERR_WORKSPACE;
  const ReduceParams rp = make_reduce_params(w, ws_base(workspace), dA, dB, dbias, d_in, d_out, r_live, grad_beta);
  memcpy(desc_out, &rp, sizeof(rp));
  *blocks_out = (d_in + 3) / 4 + (d_out + 3) / 4;
  return SOW_OK;
}

int sow_reduce_batch(const void* descs, const int* starts, int n, int total_blocks, int dtype, void* stream) {
  bool pf;
  const int cd = split_dtype(dtype, &pf);
  if (cd < 0) return SOW_ERR_DTYPE;
  if (pf) dtype = SOW_F32;   // the slab partials are fp32 whatever the compute dtype: fp32 gradients are their sums, rounded once
  if (n < 0 || total_blocks < 0) return SOW_ERR_SHAPE;
  if (n == 0) return SOW_OK;
  if (!descs || !starts) return SOW_ERR_NULL;
  return launch_tn_reduce_batch((const ReduceParams*)descs, starts, n, total_blocks, dtype, (hipStream_t)stream);
}

size_t sow_forward_workspace_bytes(int64_t T, int d_in, int d_out, int r_live, int r_acc, int acc_kind, int dtype) {
  bool pf;
  const bool fuse = fuse_of(dtype);
  dtype = split_dtype(dtype, &pf);
  if (T < 0 || d_in <= 0 || d_out <= 0 || r_live <= 0 || dtype < 0) return 0;
  if (pf) {   // the forward's own scratch (if any) followed by the packed parameters (pack_layer)
    const size_t own = sow_forward_workspace_bytes(T, d_in, d_out, r_live, r_acc, acc_kind, dtype);
    const size_t pack = pack_bytes(d_in, d_out, r_live, acc_kind == SOW_ACC_LOWRANK ? r_acc : 0, acc_kind);
    return own ? own + pack : pack + 256;
  }
  const bool wide_acc = acc_kind == SOW_ACC_LOWRANK && r_acc > 64;
  const WsPlan w = plan_ws(T, d_in, d_out, r_live, r_acc, acc_kind, dtype, fuse);
  if (!w.fused && !wide_acc && r_live <= 64 && short_hp_bytes(T, d_in, d_out, r_live, dtype) == 0 && w.planes_bytes == 0 && w.sk_bytes == 0)
    return 0;   // the forward does not touch it
  return w.total + 256;
}

size_t sow_workspace_bytes(int64_t T, int d_in, int d_out, int r_live, int r_acc, int acc_kind, int dtype) {
  bool pf;
  const bool fuse = fuse_of(dtype);
  dtype = split_dtype(dtype, &pf);
  if (T < 0 || d_in <= 0 || d_out <= 0 || r_live <= 0 || dtype < 0) return 0;
  const size_t pack = pf ? pack_bytes(d_in, d_out, r_live, acc_kind == SOW_ACC_LOWRANK ? r_acc : 0, acc_kind) : 0;
  return plan_ws(T, d_in, d_out, r_live, r_acc, acc_kind, dtype, fuse).total + pack + 256;
}


static int forward_impl(const void* x, const void* A, const void* B, const void* acc_down, const void* acc_up, const void* bias,
                        void* y, void* h_save, int64_t T, int d_in, int d_out, int r_live, int r_acc, int acc_kind, float scale,
                        int dtype, void* workspace, size_t workspace_bytes, void* stream_, bool fuse = false) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ok_dtype(dtype)) return SOW_ERR_DTYPE;
  if (T < 0 || d_in <= 0 || d_out <= 0 || r_live <= 0) return SOW_ERR_SHAPE;
  if (T == 0) return SOW_OK;
  if (!x || !A || !B || !y) return SOW_ERR_NULL;
  if (acc_kind != SOW_ACC_NONE && !acc_down) return SOW_ERR_NULL;
  if (acc_kind == SOW_ACC_LOWRANK && (!acc_up || r_acc <= 0)) return SOW_ERR_SHAPE;
  if (acc_kind != SOW_ACC_LOWRANK) r_acc = 0;
  const WsPlan w = plan_ws(T, d_in, d_out, r_live, r_acc, acc_kind, dtype);
  char* ws = workspace ? ws_base(workspace) : nullptr;
  float beta = 0.f;
  int rc;
  // SOW_FUSE_ACC on an admitted call: the accumulator term and the live term as one chain (chain_wide_acc.hip), y written
  // once.  Anything else falls through to the unflagged path, unchanged.
  if (fuse && !sw_on(SW_NO_FUSED_ACC) && ws && al16p(x) && al16p(y) && al16p(bias) && al16p(h_save)) {
    const WsPlan wf = plan_ws(T, d_in, d_out, r_live, r_acc, acc_kind, dtype, true);
    if (wf.fused && workspace_bytes >= wf.total + 255) {
      WideAccArgs a{};
      a.X = x, a.Y = y, a.Fa1 = acc_down, a.Fl1 = A, a.Fa2 = acc_up, a.Fl2 = B;
      a.ldfa1 = r_acc, a.ldfl1 = r_live, a.ldfa2 = d_out, a.ldfl2 = d_out;
      a.Hsave = h_save, a.bias = bias, a.M = T, a.D1 = d_in, a.D2 = d_out, a.r_acc = r_acc, a.r_live = r_live;
      a.scale = scale, a.bwd = 0, a.pack = ws + wf.off_wide, a.pack_bytes = wf.wide_bytes;
      rc = launch_chain_wide_acc(a, dtype, stream);
      if (rc != SOW_ERR_UNSUPPORTED) return rc;
    }
  }
  // ragged widths: the fused chain for the low-rank accumulator (scale 1) and the live term, X read once per term; h_save
  // holds the unscaled projection (the wide contract); a dense accumulator's product x . W_acc is written by gemm_rag first.
  // Without workspace or with views off 16 bytes, the generic kernels below.
  if (rag_layer(r_live, r_acc, acc_kind, d_in, d_out, dtype) && !sw_on(SW_NO_RAGGED) && ws && workspace_bytes >= w.total + 255 &&
      al16p(x) && al16p(y) && (!bias || al16p(bias)) && (!h_save || al4p(h_save))) {
    if (acc_kind == SOW_ACC_LOWRANK) {
      rc = wide_chain(x, y, acc_down, r_acc, acc_up, d_out, nullptr, nullptr, T, d_in, d_out, r_acc, 1.f, 1.f, 0.f, false, dtype,
                      ws, w, workspace_bytes, stream, true);
      if (rc) return rc;
      beta = 1.f;
    } else if (acc_kind == SOW_ACC_DENSE) {
      rc = rag_dense_product(x, d_in, acc_down, d_out, false, y, d_out, T, d_out, d_in, dtype, stream);
      if (rc) return rc;
      beta = 1.f;
    }
    return wide_chain(x, y, A, r_live, B, d_out, h_save, bias, T, d_in, d_out, r_live, 1.f, scale, beta, false, dtype, ws, w,
                      workspace_bytes, stream, true);
  }
  if (acc_kind == SOW_ACC_DENSE) {
    if (r_live <= 64 && h_save) {
      // one product with the low-rank term as a K-extension:  y = [x, h] . [W_acc; B] + bias,  h = scale * x . A
      // -- in one launch (h projected inside the GEMM) when d_out spans at most two column tiles
      // gemm4h: projection pass + anti-phase main loop in one launch, A read in place
      if (gemm4h_supported(x, d_in, acc_down, d_out, false, A, r_live, B, d_out, y, d_out, bias, h_save, T, d_out, d_in, r_live,
                           dtype))
        return launch_gemm4h(x, d_in, acc_down, d_out, false, A, r_live, B, d_out, y, d_out, bias, h_save, T, d_out, d_in,
                             r_live, scale, dtype, stream);
      if (gemm2h_supported(x, d_in, acc_down, d_out, false, A, r_live, B, d_out, y, d_out, bias, h_save, T, d_out, d_in,
                           r_live, dtype))
        return launch_gemm2h(x, d_in, acc_down, d_out, false, A, r_live, B, d_out, y, d_out, bias, h_save, T, d_out, d_in,
                             r_live, scale, stream);
      ChainParams ph{};
      ph.X = x, ph.Y = nullptr, ph.Hsave = h_save, ph.bias = nullptr;
      ph.M = T, ph.ldx = d_in, ph.ldy = d_out, ph.D1 = d_in, ph.D2 = 0;
      ph.F1b = A, ph.ldf1b = r_live, ph.F2b = B, ph.ldf2b = d_out, ph.rb = r_live;
      ph.scale = scale, ph.beta = 0.f;
      set_planes(ph, ws, w, workspace_bytes);
      if (chain2_supported(ph, dtype) &&
          gemm2_supported(x, d_in, acc_down, d_out, false, h_save, 64, B, d_out, y, d_out, bias, T, d_out, d_in, dtype)) {
        // short T: the H-only pass split over K (T / 64 workgroups cannot fill the chip: 29 us on 16 workgroups at 1024 x 4096)
        rc = SOW_ERR_UNSUPPORTED;
        if (ws && workspace_bytes >= w.total) rc = launch_chain_short(ph, dtype, false, (float*)(ws + w.off_hp), stream);
        if (rc == SOW_ERR_UNSUPPORTED) rc = launch_chain2(ph, false, dtype, stream);
        if (rc) return rc;
        const bool sk = ws && w.sk_bytes && workspace_bytes >= w.total;
        return launch_gemm2(x, d_in, acc_down, d_out, false, h_save, 64, B, d_out, r_live, y, d_out, bias, T, d_out, d_in,
                            1.f, 0.f, stream, sk ? ws + w.off_sk : nullptr, sk ? w.sk_bytes : 0);
      }
    }
    rc = gemm_auto(x, d_in, acc_down, d_out, false, y, d_out, nullptr, T, d_out, d_in, 1.f, 0.f, dtype, stream);
    if (rc) return rc;
    beta = 1.f;
  } else if (acc_kind == SOW_ACC_LOWRANK) {
    if (r_acc <= 64) {
      ChainParams p{};
      p.X = x, p.Y = y, p.Hsave = nullptr, p.bias = nullptr;
      p.M = T, p.ldx = d_in, p.ldy = d_out, p.D1 = d_in, p.D2 = d_out;
      p.F1b = acc_down, p.ldf1b = r_acc, p.F2b = acc_up, p.ldf2b = d_out, p.rb = r_acc;
      p.scale = 1.f, p.beta = 0.f;
      set_planes(p, ws, w, workspace_bytes);
      rc = launch_chain(p, dtype, false, stream);
      if (rc) return rc;
      beta = 1.f;
    } else {
      if (!ws || workspace_bytes < w.total) return SOW_ERR_WORKSPACE;
      rc = wide_chain(x, y, acc_down, r_acc, acc_up, d_out, nullptr, nullptr, T, d_in, d_out, r_acc, 1.f, 1.f, 0.f, false, dtype,
                      ws, w, workspace_bytes, stream);
      if (rc == SOW_ERR_UNSUPPORTED) {
        void* t = ws + w.off_t;
        rc = launch_gemm(x, d_in, false, acc_down, r_acc, false, t, r_acc, nullptr, T, r_acc, d_in, 1.f, 0.f, dtype, stream);
        if (rc) return rc;
        rc = launch_gemm(t, r_acc, false, acc_up, d_out, false, y, d_out, nullptr, T, d_out, r_acc, 1.f, 0.f, dtype, stream);
      }
      if (rc) return rc;
      beta = 1.f;
    }
  }
  if (r_live <= 64) {
    ChainParams p{};
    p.X = x, p.Y = y, p.Hsave = h_save, p.bias = bias;
    p.M = T, p.ldx = d_in, p.ldy = d_out, p.D1 = d_in, p.D2 = d_out;
    p.F1b = A, p.ldf1b = r_live, p.F2b = B, p.ldf2b = d_out, p.rb = r_live;
    p.scale = scale, p.beta = beta;
    set_planes(p, ws, w, workspace_bytes);
    if (ws && workspace_bytes >= w.total) {
      rc = launch_chain_short(p, dtype, false, (float*)(ws + w.off_hp), stream);
      if (rc != SOW_ERR_UNSUPPORTED) return rc;
    }
    return launch_chain(p, dtype, false, stream);
  }
  // wide rank: the fused chain (h = x A kept on chip, copied to h_save when given), else the generic composition
  //   h = x A ; y = beta*y + scale * h B + bias   with h in h_save or, without it, in the workspace
  const bool ws_ok = ws && workspace_bytes >= w.total + 255;
  rc = wide_chain(x, y, A, r_live, B, d_out, h_save, bias, T, d_in, d_out, r_live, 1.f, scale, beta, false, dtype, ws, w,
                  workspace_bytes, stream);
  if (rc != SOW_ERR_UNSUPPORTED) return rc;
  void* h = h_save;
  if (!h) {
    if (!ws_ok) return SOW_ERR_WORKSPACE;
    h = ws + w.off_dh;
  }
  rc = launch_gemm(x, d_in, false, A, r_live, false, h, r_live, nullptr, T, r_live, d_in, 1.f, 0.f, dtype, stream);
  if (rc) return rc;
  return launch_gemm(h, r_live, false, B, d_out, false, y, d_out, bias, T, d_out, r_live, scale, beta, dtype, stream);
}

int sow_forward(const void* x, const void* A, const void* B, const void* acc_down, const void* acc_up, const void* bias,
                void* y, void* h_save, int64_t T, int d_in, int d_out, int r_live, int r_acc, int acc_kind, float scale,
                int dtype, void* workspace, size_t workspace_bytes, void* stream) {
  bool pf;
  const int cd = split_dtype(dtype, &pf);
  if (cd < 0) return SOW_ERR_DTYPE;
  if (!pf)
    return forward_impl(x, A, B, acc_down, acc_up, bias, y, h_save, T, d_in, d_out, r_live, r_acc, acc_kind, scale, cd,
                        workspace, workspace_bytes, stream, fuse_of(dtype));
  // fp32 parameters: the same checks as forward_impl before the pack launch reads them
  if (T < 0 || d_in <= 0 || d_out <= 0 || r_live <= 0) return SOW_ERR_SHAPE;
  if (T == 0) return SOW_OK;
  if (!x || !A || !B || !y) return SOW_ERR_NULL;
  if (acc_kind != SOW_ACC_NONE && !acc_down) return SOW_ERR_NULL;
  if (acc_kind == SOW_ACC_LOWRANK && (!acc_up || r_acc <= 0)) return SOW_ERR_SHAPE;
  if (acc_kind != SOW_ACC_LOWRANK) r_acc = 0, acc_up = nullptr;
  if (acc_kind == SOW_ACC_NONE) acc_down = nullptr;
  sow_layer_args L = single_layer(A, B, acc_down, acc_up, bias, T, d_in, d_out, r_live, r_acc, acc_kind, workspace, workspace_bytes);
  std::vector<PackItem> items;
  int rc = pack_layer(L, cd, true, items);
  if (rc) return rc;
  if ((rc = launch_pack_params(items.data(), (int)items.size(), cd, (hipStream_t)stream))) return rc;
  return forward_impl(x, L.A, L.B, L.acc_down, L.acc_up, L.bias, y, h_save, T, d_in, d_out, r_live, r_acc, acc_kind, scale, cd,
                      L.workspace, L.workspace_bytes, stream);
}

// gdt: the dtype of dA / dB / dbias -- dtype, or SOW_F32 under SOW_PARAM_F32 (the fp32 slab sums rounded once to fp32)
static int backward_impl(const void* dy, const void* x, const void* h_save, const void* A, const void* B, const void* acc_down,
                         const void* acc_up, void* dx, void* dA, void* dB, void* dbias, int64_t T, int d_in, int d_out,
                         int r_live, int r_acc, int acc_kind, float scale, float grad_beta, int dtype, int gdt, void* workspace,
                         size_t workspace_bytes, int phases, void* stream_, bool fuse = false) {
  hipStream_t stream = (hipStream_t)stream_;
  bool do_data = (phases & SOW_BWD_DATA) != 0;
  const bool do_partial = (phases & (SOW_BWD_WEIGHTS | SOW_BWD_WEIGHTS_PARTIAL)) != 0;
  const bool do_reduce = (phases & (SOW_BWD_WEIGHTS | SOW_BWD_WEIGHTS_REDUCE)) != 0;
  const bool do_weights = do_partial || do_reduce;
  if (!do_data && !do_weights) return SOW_ERR_SHAPE;
  if (!ok_dtype(dtype)) return SOW_ERR_DTYPE;
  if (T < 0 || d_in <= 0 || d_out <= 0 || r_live <= 0) return SOW_ERR_SHAPE;
  if (T == 0) {
    // empty batch: gradients are zero (or unchanged when accumulating); x / dy / dx may be NULL
    if (!dA || !dB) return SOW_ERR_NULL;
    if (grad_beta == 0.f) {
      void* ptrs[3] = {dA, dB, dbias};
      int64_t bytes[3] = {(int64_t)d_in * r_live * (int64_t)esize(gdt), (int64_t)r_live * d_out * (int64_t)esize(gdt),
                          dbias ? (int64_t)d_out * (int64_t)esize(gdt) : 0};
      return launch_multi_zero(ptrs, bytes, 3, stream);
    }
    return SOW_OK;
  }
  if (!dy || !x || !h_save || !A || !B || !dx || !dA || !dB || !workspace) return SOW_ERR_NULL;
  if (acc_kind != SOW_ACC_NONE && !acc_down) return SOW_ERR_NULL;
  if (acc_kind == SOW_ACC_LOWRANK && (!acc_up || r_acc <= 0)) return SOW_ERR_SHAPE;
  if (acc_kind != SOW_ACC_LOWRANK) r_acc = 0;
  const WsPlan w = plan_ws(T, d_in, d_out, r_live, r_acc, acc_kind, dtype);
  if (workspace_bytes < w.total + 255) return SOW_ERR_WORKSPACE;
  char* ws = ws_base(workspace);
  void* dh = ws + w.off_dh;
  float beta = 0.f;
  int rc;
  bool data_done = false;
  // SOW_FUSE_ACC on an admitted call: dX of the accumulator and of the live term as one chain (chain_wide_acc.hip), dh left
  // in the workspace as the two-pass path leaves it; the weight phases below are the unflagged ones
  if (do_data && fuse && !sw_on(SW_NO_FUSED_ACC) && al16p(dy) && al16p(dx)) {
    const WsPlan wf = plan_ws(T, d_in, d_out, r_live, r_acc, acc_kind, dtype, true);
    if (wf.fused && workspace_bytes >= wf.total + 255) {
      WideAccArgs a{};
      a.X = dy, a.Y = dx, a.Fa1 = acc_up, a.Fl1 = B, a.Fa2 = acc_down, a.Fl2 = A;
      a.ldfa1 = d_out, a.ldfl1 = d_out, a.ldfa2 = r_acc, a.ldfl2 = r_live;
      a.Hsave = dh, a.bias = nullptr, a.M = T, a.D1 = d_out, a.D2 = d_in, a.r_acc = r_acc, a.r_live = r_live;
      a.scale = scale, a.bwd = 1, a.pack = ws + wf.off_wide, a.pack_bytes = wf.wide_bytes;
      rc = launch_chain_wide_acc(a, dtype, stream);
      if (rc && rc != SOW_ERR_UNSUPPORTED) return rc;
      if (!rc) do_data = false;
    }
  }
  // ragged widths: the fused chain for the data gradient (dY and dX views 16-byte aligned, else the generic kernels below:
  // they leave the same dh) and skinny_tn_wide for every weight gradient, dbias included, in the PARTIAL phase
  const bool rag_w = rag_layer(r_live, r_acc, acc_kind, d_in, d_out, dtype) && !sw_on(SW_NO_RAGGED);
  if (rag_w && do_data && al16p(dy) && al16p(dx)) {
    if (acc_kind == SOW_ACC_LOWRANK) {
      rc = wide_chain(dy, dx, acc_up, d_out, acc_down, r_acc, nullptr, nullptr, T, d_out, d_in, r_acc, 1.f, 1.f, 0.f, true, dtype,
                      ws, w, workspace_bytes, stream, true);
      if (rc) return rc;
      beta = 1.f;
    } else if (acc_kind == SOW_ACC_DENSE) {
      // dX = dY . W_acc^T   (W_acc stored [d_in, d_out] = [N, K])
      rc = rag_dense_product(dy, d_out, acc_down, d_out, true, dx, d_in, T, d_in, d_out, dtype, stream);
      if (rc) return rc;
      beta = 1.f;
    }
    rc = wide_chain(dy, dx, B, d_out, A, r_live, dh, nullptr, T, d_out, d_in, r_live, scale, 1.f, beta, true, dtype, ws, w,
                    workspace_bytes, stream, true);
    if (rc) return rc;
    do_data = false;
  }
  if (!do_data) {
    // weights-only call: dh was produced by an earlier SOW_BWD_DATA call on the same workspace
  } else if (acc_kind == SOW_ACC_DENSE) {
    if (r_live <= 64) {
      // one product with the low-rank term as a K-extension:  dX = [dY, dh] . [W_acc^T; A^T],  dh = scale * dY . B^T
      ChainParams pd{};
      pd.X = dy, pd.Y = nullptr, pd.Hsave = dh, pd.bias = nullptr;
      pd.M = T, pd.ldx = d_out, pd.ldy = d_in, pd.D1 = d_out, pd.D2 = 0;
      pd.F1b = B, pd.ldf1b = d_out, pd.F2b = A, pd.ldf2b = r_live, pd.rb = r_live;
      pd.scale = scale, pd.beta = 0.f;
      set_planes(pd, ws, w, workspace_bytes);
      void* apad = ws + w.off_apad;
      if (gemm4h_supported(dy, d_out, acc_down, d_out, true, B, d_out, A, r_live, dx, d_in, nullptr, dh, T, d_in, d_out, r_live,
                           dtype)) {
        // one launch: dh projected by the kernel's own pass over dY, A^T read from A's own 2r-byte rows
        rc = launch_gemm4h(dy, d_out, acc_down, d_out, true, B, d_out, A, r_live, dx, d_in, nullptr, dh, T, d_in, d_out, r_live,
                           scale, dtype, stream);
        if (rc) return rc;
        data_done = true;
      } else if (gemm2h_supported(dy, d_out, acc_down, d_out, true, B, d_out, A, r_live, dx, d_in, nullptr, dh, T, d_in, d_out,
                           r_live, dtype)) {
        // one launch: dh projected inside the GEMM, A^T read from A's own 2r-byte rows
        rc = launch_gemm2h(dy, d_out, acc_down, d_out, true, B, d_out, A, r_live, dx, d_in, nullptr, dh, T, d_in, d_out,
                           r_live, scale, stream);
        if (rc) return rc;
        data_done = true;
      } else if (chain2_supported(pd, dtype) &&
          gemm2_supported(dy, d_out, acc_down, d_out, true, dh, 64, apad, 64, dx, d_in, nullptr, T, d_in, d_out, dtype)) {
        // A zero-padded to 64 columns rides along in the dh launch when that grid is large enough
        const bool pad_fused = (int64_t)ceil_div(T, 64) * 64 >= d_in;
        if (pad_fused) pd.pad_src = A, pd.pad_dst = apad, pd.pad_rows = d_in, pd.pad_r = r_live;
        rc = SOW_ERR_UNSUPPORTED;
        if (short_hp_bytes(T, d_in, d_out, r_live, dtype)) rc = launch_chain_short(pd, dtype, true, (float*)(ws + w.off_hp), stream);
        if (rc == SOW_ERR_UNSUPPORTED) rc = launch_chain2(pd, true, dtype, stream);
        if (rc) return rc;
        if (!pad_fused) {
          rc = launch_pad64(A, apad, d_in, r_live, stream);
          if (rc) return rc;
        }
        rc = launch_gemm2(dy, d_out, acc_down, d_out, true, dh, 64, apad, 64, 64, dx, d_in, nullptr, T, d_in, d_out, 1.f, 0.f,
                          stream, w.sk_bytes ? ws + w.off_sk : nullptr, w.sk_bytes);
        if (rc) return rc;
        data_done = true;
      }
    }
    // dX = dY . W_acc^T   (W_acc stored [d_in, d_out] = [N, K])
    if (!data_done) rc = gemm_auto(dy, d_out, acc_down, d_out, true, dx, d_in, nullptr, T, d_in, d_out, 1.f, 0.f, dtype, stream);
    if (rc) return rc;
    beta = 1.f;
  } else if (acc_kind == SOW_ACC_LOWRANK) {
    if (r_acc <= 64) {
      // dX = (dY . R_up^T) . Q^T : the same chain kernel with the frozen factors, scale 1
      ChainParams p{};
      p.X = dy, p.Y = dx, p.Hsave = nullptr, p.bias = nullptr;
      p.M = T, p.ldx = d_out, p.ldy = d_in, p.D1 = d_out, p.D2 = d_in;
      p.F1b = acc_up, p.ldf1b = d_out, p.F2b = acc_down, p.ldf2b = r_acc, p.rb = r_acc;
      p.scale = 1.f, p.beta = 0.f;
      set_planes(p, ws, w, workspace_bytes);
      rc = launch_chain(p, dtype, true, stream);
      if (rc) return rc;
      beta = 1.f;
    } else {
      rc = wide_chain(dy, dx, acc_up, d_out, acc_down, r_acc, nullptr, nullptr, T, d_out, d_in, r_acc, 1.f, 1.f, 0.f, true, dtype,
                      ws, w, workspace_bytes, stream);
      if (rc == SOW_ERR_UNSUPPORTED) {
        void* t = ws + w.off_t;
        rc = launch_gemm(dy, d_out, false, acc_up, d_out, true, t, r_acc, nullptr, T, r_acc, d_out, 1.f, 0.f, dtype, stream);
        if (rc) return rc;
        rc = launch_gemm(t, r_acc, false, acc_down, r_acc, true, dx, d_in, nullptr, T, d_in, r_acc, 1.f, 0.f, dtype, stream);
      }
      if (rc) return rc;
      beta = 1.f;
    }
  }
  if (r_live <= 64) {
    ChainParams p{};
    p.X = dy, p.Y = dx, p.Hsave = dh, p.bias = nullptr;
    p.M = T, p.ldx = d_out, p.ldy = d_in, p.D1 = d_out, p.D2 = d_in;
    p.F1b = B, p.ldf1b = d_out, p.F2b = A, p.ldf2b = r_live, p.rb = r_live;
    p.scale = scale, p.beta = beta;
    set_planes(p, ws, w, workspace_bytes);
    if (do_data && !data_done) {
      rc = launch_chain_short(p, dtype, true, short_hp_bytes(T, d_in, d_out, r_live, dtype) ? (float*)(ws + w.off_hp) : nullptr, stream);
      if (rc == SOW_ERR_UNSUPPORTED) rc = launch_chain(p, dtype, true, stream);
      if (rc) return rc;
    }
    if (!do_weights) return SOW_OK;
    // weight gradients: dA = x^T dh ; dB^T = dY^T h ; dbias = colsum(dY) via the all-ones column 63
    const bool ones_ok = dbias && r_live <= 63;
    TnParams tp{};
    tp.njobs = 2, tp.T = T, tp.ns = w.ns, tp.slab_len = w.slab_len;
    auto vec_ok = [&](const void* ptr, int D) {
      if (dtype == SOW_F32) return (D % 4 == 0 && al16p(ptr)) ? 1 : 0;
      return (D % 2 == 0 && al4p(ptr)) ? 1 : 0;
    };
    // the chain kernels write 1.0 into column 63 of h_save / dh whenever r_live <= 63
    tp.job[0] = TnJob{x, dh, (float*)(ws + w.off_p0), (int64_t)d_in, d_in, -1, (d_in + 63) / 64, vec_ok(x, d_in), 1};
    tp.job[1] = TnJob{dy, h_save, (float*)(ws + w.off_p1), (int64_t)d_out, d_out, ones_ok ? 63 : -1, (d_out + 63) / 64,
                      vec_ok(dy, d_out), 1};
    if (do_partial) {
      rc = launch_tn(tp, dtype, stream);
      if (rc) return rc;
    }
    if (!do_reduce) return SOW_OK;
    const ReduceParams rp = make_reduce_params(w, ws, dA, dB, ones_ok ? dbias : nullptr, d_in, d_out, r_live, grad_beta);
    rc = launch_tn_reduce(rp, gdt, stream);
    if (rc) return rc;
    if (dbias && !ones_ok) {
      rc = launch_colsum(dy, T, d_out, dbias, grad_beta, dtype, gdt, stream);
      if (rc) return rc;
    }
    return SOW_OK;
  }
  // wide rank: the fused chain (dh = scale dY B^T to the workspace, dX = beta dX + dh A^T) and the token-slab weight-gradient
  // kernel, else the generic GEMM composition
  if (do_data) {
    rc = wide_chain(dy, dx, B, d_out, A, r_live, dh, nullptr, T, d_out, d_in, r_live, scale, 1.f, beta, true, dtype, ws, w,
                    workspace_bytes, stream);
    if (rc == SOW_ERR_UNSUPPORTED) {
      rc = launch_gemm(dy, d_out, false, B, d_out, true, dh, r_live, nullptr, T, r_live, d_out, scale, 0.f, dtype, stream);
      if (rc) return rc;
      rc = launch_gemm(dh, r_live, false, A, r_live, true, dx, d_in, nullptr, T, d_in, r_live, 1.f, beta, dtype, stream);
    }
    if (rc) return rc;
  }
  if (!do_partial) return SOW_OK;   // wide ranks: the PARTIAL phase does all of the weight gradients
  if (w.pw_bytes && (rag_w || (!sw_on(SW_NO_WIDE_CHAIN) && tnw_shape_ok(r_live, d_in, d_out, dtype)))) {
    rc = launch_tn_wide(x, dh, dy, h_save, dA, dB, dbias, T, d_in, d_out, r_live, scale, grad_beta, dtype, gdt, ws + w.off_pw,
                        w.pw_bytes, stream);
    if (rc != SOW_ERR_UNSUPPORTED) return rc;
  }
  rc = launch_gemm_out(x, d_in, true, dh, r_live, false, dA, r_live, nullptr, d_in, r_live, (int)T, 1.f, grad_beta, dtype, gdt,
                       stream);
  if (rc) return rc;
  rc = launch_gemm_out(h_save, r_live, true, dy, d_out, false, dB, d_out, nullptr, r_live, d_out, (int)T, scale, grad_beta, dtype,
                       gdt, stream);
  if (rc) return rc;
  if (dbias) {
    rc = launch_colsum(dy, T, d_out, dbias, grad_beta, dtype, gdt, stream);
    if (rc) return rc;
  }
  return SOW_OK;
}

int sow_backward_ex(const void* dy, const void* x, const void* h_save, const void* A, const void* B, const void* acc_down,
                    const void* acc_up, void* dx, void* dA, void* dB, void* dbias, int64_t T, int d_in, int d_out,
                    int r_live, int r_acc, int acc_kind, float scale, float grad_beta, int dtype, void* workspace,
                    size_t workspace_bytes, int phases, void* stream) {
  bool pf;
  const int cd = split_dtype(dtype, &pf);
  if (!pf)
    return backward_impl(dy, x, h_save, A, B, acc_down, acc_up, dx, dA, dB, dbias, T, d_in, d_out, r_live, r_acc, acc_kind, scale,
                         grad_beta, nofuse(dtype), nofuse(dtype), workspace, workspace_bytes, phases, stream, fuse_of(dtype));
  if (cd < 0) return SOW_ERR_DTYPE;
  // fp32 parameters: only the data gradient reads the factors (and the accumulator); they are packed when it runs
  if ((phases & SOW_BWD_DATA) && T > 0) {
    if (d_in <= 0 || d_out <= 0 || r_live <= 0) return SOW_ERR_SHAPE;
    if (!dy || !x || !h_save || !A || !B || !dx || !dA || !dB || !workspace) return SOW_ERR_NULL;
    if (acc_kind != SOW_ACC_NONE && !acc_down) return SOW_ERR_NULL;
    if (acc_kind == SOW_ACC_LOWRANK && (!acc_up || r_acc <= 0)) return SOW_ERR_SHAPE;
    if (acc_kind != SOW_ACC_LOWRANK) r_acc = 0, acc_up = nullptr;
    if (acc_kind == SOW_ACC_NONE) acc_down = nullptr;
    sow_layer_args L = single_layer(A, B, acc_down, acc_up, nullptr, T, d_in, d_out, r_live, r_acc, acc_kind, workspace,
                                    workspace_bytes);
    std::vector<PackItem> items;
    int rc = pack_layer(L, cd, false, items);
    if (rc) return rc;
    if ((rc = launch_pack_params(items.data(), (int)items.size(), cd, (hipStream_t)stream))) return rc;
    A = L.A, B = L.B, acc_down = L.acc_down, acc_up = L.acc_up;
  }
  return backward_impl(dy, x, h_save, A, B, acc_down, acc_up, dx, dA, dB, dbias, T, d_in, d_out, r_live, r_acc, acc_kind, scale,
                       grad_beta, cd, SOW_F32, workspace, workspace_bytes, phases, stream);
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
// TN_MAXG at a time; every other layer is forwarded to the single-layer entry point.  Results are bit-identical to n
// separate calls: the shared grid runs each layer's own workgroups unchanged.
static bool group_chain_params(const sow_layer_args& L, bool bwd, int dtype, const WsPlan& w, ChainParams* out) {
  if ((dtype != SOW_BF16 && dtype != SOW_F16) || L.acc_kind != SOW_ACC_NONE || L.r_live > 64 || sw_on(SW_NO_GROUPED) || sw_on(SW_FORCE_CHAIN_V1))
    return false;
  if (ceil_div(L.T, 64) <= SHORT_NTB) return false;   // short inputs: K / column split, single-layer path
  ChainParams p{};
  if (!bwd) {
    p.X = L.x, p.Y = L.y, p.Hsave = L.h_save, p.bias = L.bias;
    p.M = L.T, p.ldx = L.d_in, p.ldy = L.d_out, p.D1 = L.d_in, p.D2 = L.d_out;
    p.F1b = L.A, p.ldf1b = L.r_live, p.F2b = L.B, p.ldf2b = L.d_out, p.rb = L.r_live;
  } else {
    p.X = L.dy, p.Y = L.dx, p.Hsave = ws_base(L.workspace) + w.off_dh, p.bias = nullptr;
    p.M = L.T, p.ldx = L.d_out, p.ldy = L.d_in, p.D1 = L.d_out, p.D2 = L.d_in;
    p.F1b = L.B, p.ldf1b = L.d_out, p.F2b = L.A, p.ldf2b = L.r_live, p.rb = L.r_live;
  }
  p.scale = L.scale, p.beta = 0.f;
  if (!chain2_supported(p, dtype)) return false;
  // the alignment conditions launch_chain2 would reject (it then falls back inside launch_chain)
  const void* Bp = bwd ? p.F1b : p.F2b;
  const int64_t ldB = bwd ? p.ldf1b : p.ldf2b;
  const void* Ap = bwd ? p.F2b : p.F1b;
  if ((reinterpret_cast<uintptr_t>(Bp) & 15) || ldB % 8 || (reinterpret_cast<uintptr_t>(Ap) & 3)) return false;
  *out = p;
  return true;
}

// Group-planned slab counts for the weight-gradient partial sums (skinny_tn.hip: tn_partial_rows_kernel).  A pure function
// of the layer list, so that sow_backward_group and sow_backward_group_reduce_desc agree.  Items 2 i, 2 i + 1 = the two
// operands (x with dh, dY with h) of layer i.
// f16 takes the plan only when the caller asks for it (SOW_BWD_GROUP_SLABS: a deferred reduction); a call that runs both
// weight phases itself keeps the column-owner kernel for f16, whose grouped results are pinned bit-identical to single calls.
static bool group_rows_plan(const sow_layer_args* layers, int n, int dtype, int phases, int* ns, int* slab_len) {
  if (!tn_dma_dtype(dtype) || (dtype == SOW_F16 && !(phases & SOW_BWD_GROUP_SLABS)) || n < 1 || n > TN_MAXG) return false;
  int64_t T[TNR_MAXI];
  int D[TNR_MAXI], cap[TNR_MAXI];
  for (int i = 0; i < n; ++i) {
    const sow_layer_args& L = layers[i];
    if (L.T <= 0 || L.r_live > 64 || (L.dbias && L.r_live > 63)) return false;
    const WsPlan w = plan_ws(L.T, L.d_in, L.d_out, L.r_live, L.acc_kind == SOW_ACC_LOWRANK ? L.r_acc : 0, L.acc_kind, dtype);
    if (L.workspace_bytes < w.total + 255) return false;
    if (L.d_in % 8 || L.d_out % 8 || !al16p(L.x) || !al16p(L.dy) || !al16p(L.h_save)) return false;
    T[2 * i] = T[2 * i + 1] = L.T;
    D[2 * i] = L.d_in, D[2 * i + 1] = L.d_out;
    cap[2 * i] = cap[2 * i + 1] = w.ns_cap;
  }
  return tn_rows_plan(T, D, cap, 2 * n, ns, slab_len);
}

static int check_layer(const sow_layer_args& L, bool bwd) {
  if (L.T < 0 || L.d_in <= 0 || L.d_out <= 0 || L.r_live <= 0) return SOW_ERR_SHAPE;
  if (L.T == 0) return SOW_OK;
  if (!L.x || !L.A || !L.B) return SOW_ERR_NULL;
  if (!bwd && !L.y) return SOW_ERR_NULL;
  if (bwd && (!L.dy || !L.h_save || !L.dx || !L.dA || !L.dB || !L.workspace)) return SOW_ERR_NULL;
  if (L.acc_kind != SOW_ACC_NONE && !L.acc_down) return SOW_ERR_NULL;
  return SOW_OK;
}

// fp32 parameters of a group: a copy of the layer list pointing at the packed operands, every layer packed by ONE launch
static int pack_group(const sow_layer_args* layers, int n, int cd, bool bwd, std::vector<sow_layer_args>& out, void* stream) {
  out.assign(layers, layers + n);
  std::vector<PackItem> items;
  int rc;
  for (sow_layer_args& L : out) {
    if ((rc = check_layer(L, bwd))) return rc;
    if (L.T == 0) continue;
    if (L.acc_kind == SOW_ACC_LOWRANK && (!L.acc_up || L.r_acc <= 0)) return SOW_ERR_SHAPE;
    if (L.acc_kind != SOW_ACC_LOWRANK) L.acc_up = nullptr;
    if (L.acc_kind == SOW_ACC_NONE) L.acc_down = nullptr;
    if (bwd) L.bias = nullptr;   // backward reads no bias
    if ((rc = pack_layer(L, cd, !bwd, items))) return rc;
  }
  return launch_pack_params(items.data(), (int)items.size(), cd, (hipStream_t)stream);
}

static int forward_group_impl(const sow_layer_args* layers, int n, int dtype, void* stream_, bool fuse = false) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ok_dtype(dtype)) return SOW_ERR_DTYPE;
  if (n < 0) return SOW_ERR_SHAPE;
  if (n == 0) return SOW_OK;
  if (!layers) return SOW_ERR_NULL;
  ChainParams batch[C2_MAXG];
  Gemm2hArgs gbatch[4];
  int nb = 0, ng = 0, rc;
  for (int i = 0; i < n; ++i) {
    const sow_layer_args& L = layers[i];
    if ((rc = check_layer(L, false))) return rc;
    if (L.T == 0) continue;
    const WsPlan w{};
    if (group_chain_params(L, false, dtype, w, &batch[nb])) {   // h_save may be NULL (no backward follows)
      if (++nb == C2_MAXG) {
        if ((rc = launch_chain2_group(batch, nb, false, dtype, stream))) return rc;
        nb = 0;
      }
      continue;
    }
    // dense accumulator: gemm4h (one launch per layer) where it applies
    if (L.acc_kind == SOW_ACC_DENSE && L.r_live <= 64 && L.h_save &&
        gemm4h_supported(L.x, L.d_in, L.acc_down, L.d_out, false, L.A, L.r_live, L.B, L.d_out, L.y, L.d_out, L.bias, L.h_save, L.T,
                         L.d_out, L.d_in, L.r_live, dtype)) {
      if ((rc = launch_gemm4h(L.x, L.d_in, L.acc_down, L.d_out, false, L.A, L.r_live, L.B, L.d_out, L.y, L.d_out, L.bias, L.h_save,
                              L.T, L.d_out, L.d_in, L.r_live, L.scale, dtype, stream)))
        return rc;
      continue;
    }
    // dense accumulator, one launch per layer (gemm2h): the layers of a group share the grid
    if (L.acc_kind == SOW_ACC_DENSE && L.r_live <= 64 && L.h_save && !sw_on(SW_NO_GROUPED) &&
        gemm2h_supported(L.x, L.d_in, L.acc_down, L.d_out, false, L.A, L.r_live, L.B, L.d_out, L.y, L.d_out, L.bias, L.h_save, L.T,
                         L.d_out, L.d_in, L.r_live, dtype)) {
      gbatch[ng] = Gemm2hArgs{L.x, L.acc_down, L.A, L.B, L.y, L.bias, L.h_save, L.T, L.d_in, L.d_out, L.r_live, L.d_out, L.d_out,
                              L.d_out, L.d_in, L.r_live, L.scale};
      if (++ng == 4) {
        if ((rc = launch_gemm2h_group(gbatch, ng, false, stream))) return rc;
        ng = 0;
      }
      continue;
    }
    rc = sow_forward(L.x, L.A, L.B, L.acc_down, L.acc_up, L.bias, L.y, L.h_save, L.T, L.d_in, L.d_out, L.r_live, L.r_acc,
                     L.acc_kind, L.scale, fuse ? dtype | SOW_FUSE_ACC : dtype, L.workspace, L.workspace_bytes, stream_);
    if (rc) return rc;
  }
  if (ng && (rc = launch_gemm2h_group(gbatch, ng, false, stream))) return rc;
  return nb ? launch_chain2_group(batch, nb, false, dtype, stream) : SOW_OK;
}

int sow_forward_group(const sow_layer_args* layers, int n, int dtype, void* stream) {
  bool pf;
  const int cd = split_dtype(dtype, &pf);
  if (cd < 0) return SOW_ERR_DTYPE;
  if (!pf || n <= 0 || !layers) return forward_group_impl(layers, n, cd, stream, fuse_of(dtype));
  std::vector<sow_layer_args> packed;
  const int rc = pack_group(layers, n, cd, false, packed, stream);
  return rc ? rc : forward_group_impl(packed.data(), n, cd, stream);
}

// ---- generation-sized forwards (skinny_fwd.hip) --------------------------------------------------------------
// The admitted set, decided from the shape alone: 1 <= T <= 32, bf16 / f16 without SOW_PARAM_F32, a dense accumulator or none,
// r_live <= 64, widths multiples of 8.
static bool skinny_shape_ok(int64_t T, int d_in, int d_out, int r_live, int acc_kind, int dtype) {
  return (dtype == SOW_BF16 || dtype == SOW_F16) && T >= 1 && T <= 32 && d_in > 0 && d_out > 0 && r_live >= 1 && r_live <= 64 &&
         (acc_kind == SOW_ACC_DENSE || acc_kind == SOW_ACC_NONE) && d_in % 8 == 0 && d_out % 8 == 0;
}
struct SkWs {
  size_t off_py, off_ph, total;
};
static SkWs skinny_ws(int64_t T, int d_in, int d_out, int acc_kind) {
  int S, KS, ncr;
  skinny_plan(d_in, d_out, acc_kind, &S, &KS, &ncr);
  SkWs w;
  w.off_py = 0;
  w.off_ph = acc_kind == SOW_ACC_DENSE ? al256(skinny_py_bytes(T, d_out, S)) : 0;
  w.total = 256 + w.off_ph + al256(skinny_ph_bytes(T, S));
  return w;
}

size_t sow_forward_skinny_workspace_bytes(int64_t T, int d_in, int d_out, int r_live, int acc_kind, int dtype) {
  dtype = nofuse(dtype);
  if (!skinny_shape_ok(T, d_in, d_out, r_live, acc_kind, dtype)) return 0;
  return skinny_ws(T, d_in, d_out, acc_kind).total;
}

int sow_forward_skinny(const sow_layer_args* layers, int n, int dtype, void* stream) {
  bool pf;
  const int cd = split_dtype(dtype, &pf);
  if (cd < 0 || cd == SOW_F32) return SOW_ERR_DTYPE;
  if (pf || sw_on(SW_NO_SKINNY)) return SOW_ERR_UNSUPPORTED;
  if (n < 0) return SOW_ERR_SHAPE;
  if (n == 0) return SOW_OK;
  if (!layers) return SOW_ERR_NULL;
  if (n > SK_MAXL) return SOW_ERR_UNSUPPORTED;
  SkLayer sk[SK_MAXL];
  int m = 0;
  // every layer is checked before the first launch: a refusal leaves all outputs and workspaces untouched
  for (int i = 0; i < n; ++i) {
    const sow_layer_args& L = layers[i];
    if (L.T < 0 || L.d_in <= 0 || L.d_out <= 0 || L.r_live <= 0) return SOW_ERR_SHAPE;
    if (L.acc_kind != SOW_ACC_NONE && L.acc_kind != SOW_ACC_LOWRANK && L.acc_kind != SOW_ACC_DENSE) return SOW_ERR_SHAPE;
    if (L.T == 0) continue;
    if (!skinny_shape_ok(L.T, L.d_in, L.d_out, L.r_live, L.acc_kind, cd)) return SOW_ERR_UNSUPPORTED;
    const bool dense = L.acc_kind == SOW_ACC_DENSE;
    if (!L.x || !L.A || !L.B || !L.y || (dense && !L.acc_down)) return SOW_ERR_NULL;
    if (!al16p(L.x) || !al16p(L.y) || !al16p(L.A) || !al16p(L.B) || !al16p(L.bias) || (dense && !al16p(L.acc_down)))
      return SOW_ERR_UNSUPPORTED;
    const SkWs w = skinny_ws(L.T, L.d_in, L.d_out, L.acc_kind);
    if (!L.workspace || L.workspace_bytes < w.total) return SOW_ERR_WORKSPACE;
    char* ws = ws_base(L.workspace);
    SkLayer& K = sk[m++];
    K = SkLayer{};
    K.x = L.x, K.W = dense ? L.acc_down : nullptr, K.A = L.A, K.B = L.B, K.bias = L.bias, K.y = L.y;
    K.Py = dense ? (float*)(ws + w.off_py) : nullptr, K.Ph = (float*)(ws + w.off_ph);
    K.T = (int)L.T, K.d_in = L.d_in, K.d_out = L.d_out, K.r = L.r_live, K.scale = L.scale;
  }
  return launch_skinny_fwd(sk, m, cd, (hipStream_t)stream);
}

static int backward_group_impl(const sow_layer_args* layers, int n, int dtype, int gdt, int phases, void* stream_,
                               bool fuse = false) {
  hipStream_t stream = (hipStream_t)stream_;
  const bool do_data = (phases & SOW_BWD_DATA) != 0;
  const bool do_partial = (phases & (SOW_BWD_WEIGHTS | SOW_BWD_WEIGHTS_PARTIAL)) != 0;
  const bool do_reduce = (phases & (SOW_BWD_WEIGHTS | SOW_BWD_WEIGHTS_REDUCE)) != 0;
  if (!do_data && !do_partial && !do_reduce) return SOW_ERR_SHAPE;
  if (!ok_dtype(dtype)) return SOW_ERR_DTYPE;
  if (n < 0) return SOW_ERR_SHAPE;
  if (n == 0) return SOW_OK;
  if (!layers) return SOW_ERR_NULL;
  int rc;
  for (int i = 0; i < n; ++i)
    if ((rc = check_layer(layers[i], true))) return rc;
  auto single = [&](const sow_layer_args& L, int ph) {
    return backward_impl(L.dy, L.x, L.h_save, L.A, L.B, L.acc_down, L.acc_up, L.dx, L.dA, L.dB, L.dbias, L.T, L.d_in, L.d_out,
                         L.r_live, L.r_acc, L.acc_kind, L.scale, L.grad_beta, dtype, gdt, L.workspace, L.workspace_bytes, ph,
                         stream_, fuse);
  };
  auto plan = [&](const sow_layer_args& L) {
    return plan_ws(L.T, L.d_in, L.d_out, L.r_live, L.acc_kind == SOW_ACC_LOWRANK ? L.r_acc : 0, L.acc_kind, dtype);
  };
  if (do_data) {
    ChainParams batch[C2_MAXG];
    Gemm2hArgs gbatch[4];
    int nb = 0, ng = 0;
    for (int i = 0; i < n; ++i) {
      const sow_layer_args& L = layers[i];
      if (L.T == 0) {
        if ((rc = single(L, SOW_BWD_DATA | (phases & ~SOW_BWD_DATA)))) return rc;   // empty batch: everything at once
        continue;
      }
      const WsPlan w = plan(L);
      if (L.workspace_bytes < w.total + 255) return SOW_ERR_WORKSPACE;
      void* dh = ws_base(L.workspace) + w.off_dh;
      if (group_chain_params(L, true, dtype, w, &batch[nb])) {
        if (++nb == C2_MAXG) {
          if ((rc = launch_chain2_group(batch, nb, true, dtype, stream))) return rc;
          nb = 0;
        }
      } else if (L.acc_kind == SOW_ACC_DENSE && L.r_live <= 64 &&
                 gemm4h_supported(L.dy, L.d_out, L.acc_down, L.d_out, true, L.B, L.d_out, L.A, L.r_live, L.dx, L.d_in, nullptr, dh,
                                  L.T, L.d_in, L.d_out, L.r_live, dtype)) {
        if ((rc = launch_gemm4h(L.dy, L.d_out, L.acc_down, L.d_out, true, L.B, L.d_out, L.A, L.r_live, L.dx, L.d_in, nullptr, dh,
                                L.T, L.d_in, L.d_out, L.r_live, L.scale, dtype, stream)))
          return rc;
      } else if (L.acc_kind == SOW_ACC_DENSE && L.r_live <= 64 && !sw_on(SW_NO_GROUPED) &&
                 gemm2h_supported(L.dy, L.d_out, L.acc_down, L.d_out, true, L.B, L.d_out, L.A, L.r_live, L.dx, L.d_in, nullptr, dh,
                                  L.T, L.d_in, L.d_out, L.r_live, dtype)) {
        gbatch[ng] = Gemm2hArgs{L.dy, L.acc_down, L.B, L.A, L.dx, nullptr, dh, L.T, L.d_out, L.d_out, L.d_out, L.r_live, L.d_in,
                                L.d_in, L.d_out, L.r_live, L.scale};
        if (++ng == 4) {
          if ((rc = launch_gemm2h_group(gbatch, ng, true, stream))) return rc;
          ng = 0;
        }
      } else if ((rc = single(L, SOW_BWD_DATA)))
        return rc;
    }
    if (ng && (rc = launch_gemm2h_group(gbatch, ng, true, stream))) return rc;
    if (nb && (rc = launch_chain2_group(batch, nb, true, dtype, stream))) return rc;
  }
  // row-owner weight-gradient kernel with slab counts planned over the group: when the caller asks for it (and then builds
  // the deferred reduction from sow_backward_group_reduce_desc), or when this call runs the reduction itself
  int rns[TNR_MAXI], rslab[TNR_MAXI];
  const bool rows = (do_partial || do_reduce) && ((phases & SOW_BWD_GROUP_SLABS) || (do_partial && do_reduce)) &&
                    group_rows_plan(layers, n, dtype, phases, rns, rslab);
  if (do_partial && rows) {
    TnRowsItem items[TNR_MAXI];
    for (int i = 0; i < n; ++i) {
      const sow_layer_args& L = layers[i];
      const WsPlan w = plan(L);
      char* ws = ws_base(L.workspace);
      items[2 * i] = TnRowsItem{L.x, ws + w.off_dh, (float*)(ws + w.off_p0), (int64_t)L.d_in, L.T, L.d_in, 0, 0, 0, 0, rns[2 * i],
                                rslab[2 * i], 0};
      items[2 * i + 1] = TnRowsItem{L.dy, L.h_save, (float*)(ws + w.off_p1), (int64_t)L.d_out, L.T, L.d_out, 0, 0, 0, 0,
                                    rns[2 * i + 1], rslab[2 * i + 1], 0};
    }
    if ((rc = launch_tn_rows(items, 2 * n, dtype, stream))) return rc;
  } else if (do_partial) {
    TnParams batch[TN_MAXG];
    int nb = 0;
    for (int i = 0; i < n; ++i) {
      const sow_layer_args& L = layers[i];
      if (L.T == 0) {
        if (!do_data && (rc = single(L, phases))) return rc;
        continue;
      }
      const WsPlan w = plan(L);
      if (L.workspace_bytes < w.total + 255) return SOW_ERR_WORKSPACE;
      bool grouped = false;
      if (L.r_live <= 64 && !sw_on(SW_NO_GROUPED)) {
        char* ws = ws_base(L.workspace);
        TnParams tp{};
        tp.njobs = 2, tp.T = L.T, tp.ns = w.ns, tp.slab_len = w.slab_len;
        const bool ones_ok = L.dbias && L.r_live <= 63;
        const int vx = (L.d_in % 2 == 0 && al4p(L.x)) ? 1 : 0, vy = (L.d_out % 2 == 0 && al4p(L.dy)) ? 1 : 0;
        tp.job[0] = TnJob{L.x, ws + w.off_dh, (float*)(ws + w.off_p0), (int64_t)L.d_in, L.d_in, -1, (L.d_in + 63) / 64, vx, 1};
        tp.job[1] = TnJob{L.dy, L.h_save, (float*)(ws + w.off_p1), (int64_t)L.d_out, L.d_out, ones_ok ? 63 : -1,
                          (L.d_out + 63) / 64, vy, 1};
        if (tn_group_supported(tp, dtype)) {
          batch[nb] = tp;
          grouped = true;
          if (++nb == TN_MAXG) {
            if ((rc = launch_tn_group(batch, nb, dtype, stream))) return rc;
            nb = 0;
          }
        }
      }
      if (!grouped && (rc = single(L, SOW_BWD_WEIGHTS_PARTIAL))) return rc;
    }
    if (nb && (rc = launch_tn_group(batch, nb, dtype, stream))) return rc;
  }
  if (do_reduce && rows) {
    for (int i = 0; i < n; ++i) {
      const sow_layer_args& L = layers[i];
      ReduceParams rp = make_reduce_params(plan(L), ws_base(L.workspace), L.dA, L.dB, L.dbias, L.d_in, L.d_out, L.r_live, L.grad_beta);
      rp.job[0].ns = rns[2 * i], rp.job[1].ns = rns[2 * i + 1];
      if ((rc = launch_tn_reduce(rp, gdt, stream))) return rc;
    }
  } else if (do_reduce) {
    for (int i = 0; i < n; ++i)
      if (layers[i].T != 0 && (rc = single(layers[i], SOW_BWD_WEIGHTS_REDUCE))) return rc;
  }
  return SOW_OK;
}

int sow_backward_group(const sow_layer_args* layers, int n, int dtype, int phases, void* stream) {
  bool pf;
  const int cd = split_dtype(dtype, &pf);
  if (!pf) return backward_group_impl(layers, n, nofuse(dtype), nofuse(dtype), phases, stream, fuse_of(dtype));
  if (cd < 0) return SOW_ERR_DTYPE;
  if (n <= 0 || !layers || !(phases & SOW_BWD_DATA)) return backward_group_impl(layers, n, cd, SOW_F32, phases, stream);
  std::vector<sow_layer_args> packed;
  const int rc = pack_group(layers, n, cd, true, packed, stream);
  return rc ? rc : backward_group_impl(packed.data(), n, cd, SOW_F32, phases, stream);
}

// ---- shared-input entry points (chain2_shared.hip) -----------------------------------------------------------------
// Sibling layers on one x: the forward reads x once, the data gradient writes ONE dX.  Admitted: a set that
// group_chain_params takes layer by layer (bf16 / f16, no accumulator, r_live <= 64, T > 8192, chain2 alignment) with one x
// pointer and one d_in; anything else returns SOW_ERR_UNSUPPORTED before anything is launched.
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
  dtype = nofuse(dtype);
  if (!ok_dtype(dtype & ~SOW_PARAM_F32)) return SOW_ERR_DTYPE;
  int rc;
  if ((rc = shared_common(layers, n, false))) return rc;
  for (int i = 0; i < n; ++i)
    if ((rc = check_layer(layers[i], false))) return rc;
  if (sw_on(SW_NO_SHARED_X) || flagged(dtype) || n > C2_MAXG || layers[0].T == 0) return SOW_ERR_UNSUPPORTED;
  ChainParams ps[C2_MAXG];
  for (int i = 0; i < n; ++i)
    if (!group_chain_params(layers[i], false, dtype, WsPlan{}, &ps[i])) return SOW_ERR_UNSUPPORTED;
  return launch_chain2_shared(ps, n, false, dtype, (hipStream_t)stream);
}

int sow_backward_shared(const sow_layer_args* layers, int n, int dtype, int phases, void* stream) {
  dtype = nofuse(dtype);
  if (!ok_dtype(dtype & ~SOW_PARAM_F32)) return SOW_ERR_DTYPE;
  int rc;
  if ((rc = shared_common(layers, n, true))) return rc;
  if (n > C2_MAXG) return SOW_ERR_UNSUPPORTED;
  if (flagged(dtype)) return SOW_ERR_UNSUPPORTED;
  sow_layer_args filled[C2_MAXG];
  shared_fill_dx(layers, n, filled);
  if (!(phases & SOW_BWD_DATA)) return sow_backward_group(filled, n, dtype, phases, stream);
  for (int i = 0; i < n; ++i)
    if ((rc = check_layer(filled[i], true))) return rc;
  if (sw_on(SW_NO_SHARED_X) || filled[0].T == 0) return SOW_ERR_UNSUPPORTED;
  ChainParams ps[C2_MAXG];
  for (int i = 0; i < n; ++i) {
    const sow_layer_args& L = filled[i];
    const WsPlan w = plan_ws(L.T, L.d_in, L.d_out, L.r_live, 0, L.acc_kind, dtype);
    if (!group_chain_params(L, true, dtype, w, &ps[i])) return SOW_ERR_UNSUPPORTED;
    if (L.workspace_bytes < w.total + 255) return SOW_ERR_WORKSPACE;
    ps[i].beta = filled[0].grad_beta;   // dX = grad_beta * dX + sum_i dh_i A_i^T
  }
  if ((rc = launch_chain2_shared(ps, n, true, dtype, (hipStream_t)stream))) return rc;
  // the weight phases read each layer's dh where the grouped data phase leaves it: exactly sow_backward_group's code
  const int wph = phases & ~SOW_BWD_DATA;
  return (wph & (SOW_BWD_WEIGHTS | SOW_BWD_WEIGHTS_PARTIAL | SOW_BWD_WEIGHTS_REDUCE))
             ? backward_group_impl(filled, n, dtype, dtype, wph, stream)
             : SOW_OK;
}

int sow_backward_group_plan(const sow_layer_args* layers, int n, int dtype, int phases, int* slabs_out) {
  bool pf;
  dtype = split_dtype(dtype, &pf);   // the plan does not depend on the parameter dtype
  if (dtype < 0) return SOW_ERR_DTYPE;
  if (n < 0) return SOW_ERR_SHAPE;
  if (n == 0) return 0;
  if (!layers) return SOW_ERR_NULL;
  int rc;
  for (int i = 0; i < n; ++i)
    if ((rc = check_layer(layers[i], true))) return rc;
  const bool do_partial = (phases & (SOW_BWD_WEIGHTS | SOW_BWD_WEIGHTS_PARTIAL)) != 0;
  const bool do_reduce = (phases & (SOW_BWD_WEIGHTS | SOW_BWD_WEIGHTS_REDUCE)) != 0;
  int rns[TNR_MAXI], rslab[TNR_MAXI];
  const bool rows = (do_partial || do_reduce) && ((phases & SOW_BWD_GROUP_SLABS) || (do_partial && do_reduce)) &&
                    group_rows_plan(layers, n, dtype, phases, rns, rslab);
  if (slabs_out)
    for (int i = 0; i < n; ++i) {
      const sow_layer_args& L = layers[i];
      int ns = 0;
      if (L.T > 0 && L.r_live <= 64)
        ns = plan_ws(L.T, L.d_in, L.d_out, L.r_live, L.acc_kind == SOW_ACC_LOWRANK ? L.r_acc : 0, L.acc_kind, dtype).ns;
      slabs_out[2 * i] = rows ? rns[2 * i] : ns;
      slabs_out[2 * i + 1] = rows ? rns[2 * i + 1] : ns;
    }
  return rows ? 1 : 0;
}

int sow_backward_group_reduce_desc(const sow_layer_args* layers, int n, int dtype, int phases, void* descs_out, int* blocks_out) {
  bool pf;
  dtype = split_dtype(dtype, &pf);
  if (dtype < 0) return SOW_ERR_DTYPE;
  if (n < 0) return SOW_ERR_SHAPE;
  if (n == 0) return SOW_OK;
  if (!layers || !descs_out || !blocks_out) return SOW_ERR_NULL;
  int rc;
  for (int i = 0; i < n; ++i)
    if ((rc = check_layer(layers[i], true))) return rc;
  int rns[TNR_MAXI], rslab[TNR_MAXI];
  const bool rows = (phases & SOW_BWD_GROUP_SLABS) && group_rows_plan(layers, n, dtype, phases, rns, rslab);
  for (int i = 0; i < n; ++i) {
    const sow_layer_args& L = layers[i];
    char* out = (char*)descs_out + (size_t)i * sizeof(ReduceParams);
    if ((rc = sow_backward_reduce_desc(L.dA, L.dB, L.dbias, L.T, L.d_in, L.d_out, L.r_live, L.r_acc, L.acc_kind, L.grad_beta, dtype,
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

int sow_cast_copy(const void* src, int64_t lds, int src_dtype, void* dst, int64_t ldd, int dst_dtype, int64_t rows,
                  int cols, void* stream) {
  src_dtype = nofuse(src_dtype), dst_dtype = nofuse(dst_dtype);
  if (flagged(src_dtype) || flagged(dst_dtype) || !ok_dtype(src_dtype) || !ok_dtype(dst_dtype)) return SOW_ERR_DTYPE;
  if (!src || !dst) return SOW_ERR_NULL;
  return launch_cast_copy(src, lds, src_dtype, dst, ldd, dst_dtype, rows, cols, (hipStream_t)stream);
}

}  // extern "C"
