// Global gradient statistics of one flat buffer (FactorBucket.flat_grad): the sum of squares, and from it the record
// (sow_grad_stats, include/sow_amd.h) that sow_adamw_flat_seg_stats reads its gradient multiplier and its go / no-go flag
// from -- torch.nn.utils.clip_grad_norm_ (simple_train.py:631, the Trainer's max_grad_norm) and the overflow check of an
// fp16 loop without a second pass over the gradients, without rounding a scaled gradient and without a host read.
//   * grad_sumsq_partial_kernel<T>   one double per workgroup into the workspace
//   * grad_stats_finalize_kernel     one workgroup: the partials, the optional device scalars, the record, the skip counters
// Two launches on the caller's stream; every byte either kernel reads was written by this call (the workspace and the record
// need no initialisation).  No atomics and no hand-off between workgroups: the bits of sumsq depend on n, the dtype and the
// data -- not on the pointer's alignment, the clock or the number of CUs.
#include "kernels.hpp"

namespace sow {

constexpr int GS_THREADS = 256;
constexpr int GS_TILE = GS_THREADS * 8;   // elements of one tile: one 16-byte load per lane of 16-bit data, two of fp32
constexpr int GS_MAX_WG = 1024;           // workgroups (= partial sums) at most

// The split of [0, n) over the workgroups, a function of n only: tiles of GS_TILE elements, `tpw` consecutive tiles per
// workgroup, `nwg` workgroups (the last one may own fewer tiles and the ragged end).
struct GradSumPlan {
  int64_t tpw;
  int nwg;
};
static GradSumPlan plan_grad_sum(int64_t n) {
  const int64_t ntiles = (n + GS_TILE - 1) / GS_TILE;
  GradSumPlan p;
  p.tpw = ntiles <= GS_MAX_WG ? 1 : (ntiles + GS_MAX_WG - 1) / GS_MAX_WG;
  p.nwg = ntiles == 0 ? 0 : (int)((ntiles + p.tpw - 1) / p.tpw);
  return p;
}

size_t grad_stats_workspace_bytes(int64_t n) {
  // the cap of the plan, not its count (which is not monotone in n: 1025 tiles take 513 workgroups of 2): min(tiles, 1024)
  const int64_t ntiles = n <= 0 ? 0 : (n + GS_TILE - 1) / GS_TILE;
  return sizeof(double) * (size_t)(ntiles < 1 ? 1 : (ntiles > GS_MAX_WG ? GS_MAX_WG : ntiles));
}

__device__ __forceinline__ double gs_wide(float v) { return (double)v; }
__device__ __forceinline__ double gs_wide(bf16_t v) { return (double)(float)v; }
__device__ __forceinline__ double gs_wide(f16_t v) { return (double)(float)v; }

// Element e of a workgroup's range (counted from the range's first element) belongs to lane (e / VE) % 256, which adds its
// square to accumulator (e % VE) % 4, vector after vector in rising e.  VEC: the lane reads its VE elements as one 16-byte
// load (the range starts on a 16-byte line); otherwise element by element -- the same elements into the same accumulators
// in the same order, so an odd pointer changes the speed and not one bit.  The last, partial vector of a range is read
// element by element in both forms.
template <typename T, bool VEC>
__device__ __forceinline__ void gs_accumulate(const T* __restrict__ g, int64_t len, double (&acc)[4]) {
  constexpr int VE = DT<T>::VE;
  const int64_t nfull = len / VE;
  struct Vec {
    alignas(16) T e[VE];
  };
  auto load = [&](int64_t k) {
    Vec v;
    if (VEC) {
      *(u32x4*)v.e = *(const u32x4*)(g + k * VE);
    } else {
#pragma unroll
      for (int j = 0; j < VE; ++j) v.e[j] = g[k * VE + j];
    }
    return v;
  };
  auto add = [&](const Vec& v) {
#pragma unroll
    for (int j = 0; j < VE; ++j) {
      const double d = gs_wide(v.e[j]);
      acc[j & 3] = fma(d, d, acc[j & 3]);
    }
  };
  int64_t k = threadIdx.x;
  // four loads in flight per lane; the squares are added in rising k either way
  for (; k + 3 * GS_THREADS < nfull; k += 4 * GS_THREADS) {
    const Vec v0 = load(k), v1 = load(k + GS_THREADS), v2 = load(k + 2 * GS_THREADS), v3 = load(k + 3 * GS_THREADS);
    add(v0), add(v1), add(v2), add(v3);
  }
  for (; k < nfull; k += GS_THREADS) add(load(k));
  // the ragged end: fewer than VE elements, owned by the lane the next vector would have gone to
  if ((int64_t)threadIdx.x == nfull % GS_THREADS) {
    for (int64_t i = nfull * VE; i < len; ++i) {
      const double d = gs_wide(g[i]);
      const int j = (int)(i - nfull * VE);
      acc[j & 3] = fma(d, d, acc[j & 3]);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(GS_THREADS) void grad_sumsq_partial_kernel(const T* __restrict__ g, int64_t n, int64_t tpw,
                                                                        double* __restrict__ partial) {
  __shared__ double red[GS_THREADS / 64];
  const int64_t lo = (int64_t)blockIdx.x * tpw * GS_TILE;
  int64_t hi = lo + tpw * GS_TILE;
  if (hi > n) hi = n;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  // lo is a multiple of GS_TILE elements (4 or 8 KiB), so every range starts on a 16-byte line when the buffer does
  if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) gs_accumulate<T, true>(g + lo, hi - lo, acc);
  else gs_accumulate<T, false>(g + lo, hi - lo, acc);
  double s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);   // a fixed butterfly: every lane ends with the same bits
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// One workgroup.  Lane t sums the partials [t * per, (t + 1) * per) in index order, the lanes are summed by the butterfly
// and the four waves in order; lane 0 forms the record in double and rounds every fp32 field once.
__global__ __launch_bounds__(GS_THREADS) void grad_stats_finalize_kernel(const double* __restrict__ partial, int npartial,
                                                                         float grad_scale, float max_norm,
                                                                         const double* extra_sumsq, const float* loss_scale,
                                                                         const float* extra_found_inf, int32_t* skip_counters,
                                                                         int n_counters, sow_grad_stats* out) {
  __shared__ double red[GS_THREADS / 64];
  __shared__ int32_t flag;
  const int per = (npartial + GS_THREADS - 1) / GS_THREADS;
  double s = 0.0;
  for (int i = threadIdx.x * per; i < (int)(threadIdx.x + 1) * per && i < npartial; ++i) s += partial[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double sumsq = (red[0] + red[1]) + (red[2] + red[3]);
    const double mult0 = loss_scale ? (double)grad_scale / (double)*loss_scale : (double)grad_scale;
    const double total_sq = mult0 * mult0 * sumsq + (extra_sumsq ? *extra_sumsq : 0.0);
    const double norm = sqrt(total_sq);
    // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1); no clipping asked for is exactly 1
    double clip = 1.0;
    if (max_norm > 0.f && max_norm < __builtin_huge_valf()) clip = fmin(1.0, (double)max_norm / (norm + 1e-6));
    const bool bad = !(fabs(total_sq) < __builtin_huge_val()) || (extra_found_inf && *extra_found_inf != 0.f);
    out->sumsq = sumsq;
    out->total_sq = total_sq;
    out->total_norm = (float)norm;
    out->clip_coef = (float)clip;
    out->grad_mult = (float)(mult0 * clip);
    out->nonfinite = bad ? 1 : 0;
    flag = bad ? 1 : 0;
  }
  __syncthreads();
  if (skip_counters && flag)
    for (int i = threadIdx.x; i < n_counters; i += GS_THREADS) skip_counters[i] += 1;
}

int launch_grad_stats(const void* grad, int64_t n, int dtype, float grad_scale, float max_norm, const double* extra_sumsq,
                      const float* loss_scale, const float* extra_found_inf, int32_t* skip_counters, int n_counters,
                      void* workspace, size_t workspace_bytes, sow_grad_stats* out, hipStream_t stream) {
  // everything is checked before the first launch
  if (n < 0 || n_counters < 0) return SOW_ERR_SHAPE;
  if (!out || !workspace || (n > 0 && !grad) || (n_counters > 0 && !skip_counters)) return SOW_ERR_NULL;
  if (dtype != SOW_F32 && dtype != SOW_BF16 && dtype != SOW_F16) return SOW_ERR_DTYPE;
  if (workspace_bytes < grad_stats_workspace_bytes(n)) return SOW_ERR_WORKSPACE;
  const GradSumPlan p = plan_grad_sum(n);
  double* partial = (double*)workspace;
  if (p.nwg > 0) {
    if (dtype == SOW_F32)
      hipLaunchKernelGGL(grad_sumsq_partial_kernel<float>, dim3(p.nwg), dim3(GS_THREADS), 0, stream, (const float*)grad, n, p.tpw, partial);
    else if (dtype == SOW_BF16)
      hipLaunchKernelGGL(grad_sumsq_partial_kernel<bf16_t>, dim3(p.nwg), dim3(GS_THREADS), 0, stream, (const bf16_t*)grad, n, p.tpw, partial);
    else
      hipLaunchKernelGGL(grad_sumsq_partial_kernel<f16_t>, dim3(p.nwg), dim3(GS_THREADS), 0, stream, (const f16_t*)grad, n, p.tpw, partial);
    SOW_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(grad_stats_finalize_kernel, dim3(1), dim3(GS_THREADS), 0, stream, partial, p.nwg, grad_scale, max_norm,
                     extra_sumsq, loss_scale, extra_found_inf, n_counters > 0 ? skip_counters : nullptr, n_counters, out);
  SOW_CHECK_LAUNCH();
  return SOW_OK;
}

}  // namespace sow
