// Small HBM-bound helper kernels around the SoW hot path.
//   * multi-tensor zero fill       -> reset_optimizer (scripts/utils/training_utils.py:257-277) and B <- 0
//                                     in SoWLinear.accumulate (sow.py:159)
//   * flat AdamW step              -> the factor parameter group of simple_train.py:502-506 as ONE launch
//   * dense Adam moment update     -> TTAdam.step's dense section (ttadam.py:89-111)
//   * TT Hadamard core product     -> TensorTrain.__mul__ (tt.py:469-475)
//   * axpby / scale                -> TTSGD p += -lr * d_p (ttsgd.py:78)
//   * parameter pack               -> the autocast cast of fp32 factors / bias / accumulator to bf16 / f16 (SOW_PARAM_F32)
#include "kernels.hpp"

namespace sow {

constexpr int MT_MAX = 48;  // tensors per multi-tensor launch (kernel-argument resident table)

struct MultiTensor {
  void* ptr[MT_MAX];
  int64_t bytes[MT_MAX];
  int n;
};

// each workgroup walks its tensor with 16-byte stores; grid.y = tensor, grid.x = chunks
__global__ __launch_bounds__(256) void multi_zero_kernel(const MultiTensor mt) {
  const int ti = blockIdx.y;
  if (ti >= mt.n) return;
  char* base = (char*)mt.ptr[ti];
  const int64_t nb = mt.bytes[ti];
  const uintptr_t addr = reinterpret_cast<uintptr_t>(base);
  const int64_t head = ((16 - (addr & 15)) & 15) < nb ? ((16 - (addr & 15)) & 15) : nb;
  const int64_t nvec = (nb - head) / 16;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
  u32x4* v = (u32x4*)(base + head);
  for (int64_t i = tid; i < nvec; i += nth) v[i] = u32x4{0, 0, 0, 0};
  const int64_t tail0 = head + nvec * 16;
  for (int64_t i = tid; i < head; i += nth) base[i] = 0;
  for (int64_t i = tail0 + tid; i < nb; i += nth) base[i] = 0;
}

int launch_multi_zero(void* const* ptrs, const int64_t* bytes, int n, hipStream_t stream) {
  for (int off = 0; off < n; off += MT_MAX) {
    MultiTensor mt;
    mt.n = n - off < MT_MAX ? n - off : MT_MAX;
    int64_t maxb = 0;
    for (int i = 0; i < mt.n; ++i) {
      mt.ptr[i] = ptrs[off + i];
      mt.bytes[i] = bytes[off + i];
      if (bytes[off + i] > maxb) maxb = bytes[off + i];
      if (bytes[off + i] < 0 || (bytes[off + i] > 0 && !ptrs[off + i])) return SOW_ERR_NULL;
    }
    if (maxb == 0) continue;
    int gx = (int)((maxb / 16 + 255) / 256);
    if (gx < 1) gx = 1;
    if (gx > 256) gx = 256;
    hipLaunchKernelGGL(multi_zero_kernel, dim3(gx, mt.n), dim3(256), 0, stream, mt);
    SOW_CHECK_LAUNCH();
  }
  return SOW_OK;
}

// ---------------------------------------------------------------------------------------------
// AdamW over one flat buffer (torch.optim.AdamW semantics, no amsgrad, maximize=False):
//   p *= 1 - lr*wd ; m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g*g ;
//   p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps)
// State m, v are fp32 or the parameter dtype (TS); math in fp32.  The scalars 1 - b, 1 - lr*wd, lr/bc1 and sqrt(bc2) are
// formed in double on the host from double betas, as torch forms them from Python floats, and rounded to fp32 once:
// 1 - b2 taken in fp32 from b2 = 0.999 rounded to fp32 is 1.3e-5 relative (216 fp32 ulp) off 0.001, an error that would
// enter v on every step.
// ---------------------------------------------------------------------------------------------
template <typename T, typename TS>
__global__ __launch_bounds__(256) void adamw_flat_kernel(T* p, const T* g, TS* m, TS* v, int64_t n, float b1, float c1,
                                                         float b2, float c2, float eps, float decay, float step_size,
                                                         float bc2_sqrt, float grad_scale) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = tid; i < n; i += nth) {
    float pv = to_f32(p[i]);
    const float gv = to_f32(g[i]) * grad_scale;
    float mv = to_f32(m[i]), vv = to_f32(v[i]);
    pv *= decay;
    mv = b1 * mv + c1 * gv;
    vv = b2 * vv + c2 * gv * gv;
    const float denom = sqrtf(vv) / bc2_sqrt + eps;
    pv -= step_size * (mv / denom);
    p[i] = from_f32<T>(pv);
    m[i] = from_f32<TS>(mv);
    v[i] = from_f32<TS>(vv);
  }
}

int launch_adamw_flat(void* p, const void* g, void* m, void* v, int64_t n, float lr, double b1, double b2, float eps,
                      float wd, int step, float grad_scale, int dtype, int state_dtype, hipStream_t stream) {
  if (n <= 0) return SOW_OK;
  if (!p || !g || !m || !v) return SOW_ERR_NULL;
  const double bc1 = 1.0 - std::pow(b1, (double)step), bc2 = 1.0 - std::pow(b2, (double)step);
  const float b1f = (float)b1, c1 = (float)(1.0 - b1), b2f = (float)b2, c2 = (float)(1.0 - b2);
  const float decay = (float)(1.0 - (double)lr * wd), step_size = (float)(lr / bc1), bc2s = (float)std::sqrt(bc2);
  int grid = (int)((n + 255) / 256);
  if (grid > 2048) grid = 2048;
#define SOW_ADAMW(T, TS) \
  hipLaunchKernelGGL((adamw_flat_kernel<T, TS>), dim3(grid), dim3(256), 0, stream, (T*)p, (const T*)g, (TS*)m, (TS*)v, n, b1f, c1, b2f, c2, eps, decay, step_size, bc2s, grad_scale)
  if (dtype == SOW_F32 && state_dtype == SOW_F32) SOW_ADAMW(float, float);
  else if (dtype == SOW_BF16 && state_dtype == SOW_BF16) SOW_ADAMW(bf16_t, bf16_t);
  else if (dtype == SOW_BF16 && state_dtype == SOW_F32) SOW_ADAMW(bf16_t, float);
  else if (dtype == SOW_F16 && state_dtype == SOW_F16) SOW_ADAMW(f16_t, f16_t);
  else if (dtype == SOW_F16 && state_dtype == SOW_F32) SOW_ADAMW(f16_t, float);
  else return SOW_ERR_DTYPE;
#undef SOW_ADAMW
  SOW_CHECK_LAUNCH();
  return SOW_OK;
}

// ---------------------------------------------------------------------------------------------
// AdamW over SEGMENTS of one flat buffer: every segment [begin, end) has its own lr, weight decay and step count (the
// factors at sow_lr with decay and a step that reset_optimizer zeroes, the biases at lr without decay: run_glue.py:796-808).
// The per-element arithmetic is adamw_flat_kernel's, statement for statement; the three scalars that depend on lr, wd and
// step come from the segment's table entry, formed on the host exactly as launch_adamw_flat forms them.  The table rides
// in the kernel arguments.  A workgroup belongs to ONE segment (blocks [block0, block0 + nblocks) of the grid) and strides
// over that segment only, so elements outside every segment are neither read nor written.
// ---------------------------------------------------------------------------------------------
constexpr int ADAMW_MAXSEG = SOW_ADAMW_MAX_SEGMENTS;   // segments per launch: 64 x 32 bytes of by-value arguments
struct AdamwSeg {
  int64_t begin, end;
  float decay, step_size, bc2_sqrt;
  int block0;   // first workgroup of this segment
};
struct AdamwSegTable {
  AdamwSeg s[ADAMW_MAXSEG];
  int n;
};
static_assert(sizeof(AdamwSegTable) + 4 * sizeof(void*) + 6 * sizeof(float) <= 4096,
              "by-value kernel arguments must stay under 4 KiB");

template <typename T, typename TS>
__global__ __launch_bounds__(256) void adamw_flat_seg_kernel(T* p, const T* g, TS* m, TS* v, const AdamwSegTable tb, float b1,
                                                             float c1, float b2, float c2, float eps, float grad_scale) {
  const int blk = blockIdx.x;
  int si = 0;
  while (si + 1 < tb.n && blk >= tb.s[si + 1].block0) ++si;   // uniform: scalar loads of the argument table
  const AdamwSeg& S = tb.s[si];
  const int nblk = (si + 1 < tb.n ? tb.s[si + 1].block0 : (int)gridDim.x) - S.block0;
  const float decay = S.decay, step_size = S.step_size, bc2_sqrt = S.bc2_sqrt;
  const int64_t end = S.end, nth = (int64_t)nblk * blockDim.x;
  for (int64_t i = S.begin + (int64_t)(blk - S.block0) * blockDim.x + threadIdx.x; i < end; i += nth) {
    float pv = to_f32(p[i]);
    const float gv = to_f32(g[i]) * grad_scale;
    float mv = to_f32(m[i]), vv = to_f32(v[i]);
    pv *= decay;
    mv = b1 * mv + c1 * gv;
    vv = b2 * vv + c2 * gv * gv;
    const float denom = sqrtf(vv) / bc2_sqrt + eps;
    pv -= step_size * (mv / denom);
    p[i] = from_f32<T>(pv);
    m[i] = from_f32<TS>(mv);
    v[i] = from_f32<TS>(vv);
  }
}

int launch_adamw_flat_seg(void* p, const void* g, void* m, void* v, const sow_adamw_segment* segs, int n_segs, double b1,
                          double b2, float eps, float grad_scale, int dtype, int state_dtype, hipStream_t stream) {
  if (n_segs < 0) return SOW_ERR_SHAPE;
  if (n_segs == 0) return SOW_OK;
  if (!p || !g || !m || !v || !segs) return SOW_ERR_NULL;
  const bool dt_ok = (dtype == SOW_F32 && state_dtype == SOW_F32) ||
                     ((dtype == SOW_BF16 || dtype == SOW_F16) && (state_dtype == dtype || state_dtype == SOW_F32));
  if (!dt_ok) return SOW_ERR_DTYPE;
  // every segment is checked before the first launch: sorted, disjoint, non-empty, step >= 1
  for (int i = 0; i < n_segs; ++i) {
    if (segs[i].begin < 0 || segs[i].end <= segs[i].begin || segs[i].step < 1) return SOW_ERR_SHAPE;
    if (i && segs[i].begin < segs[i - 1].end) return SOW_ERR_SHAPE;
  }
  const float b1f = (float)b1, c1 = (float)(1.0 - b1), b2f = (float)b2, c2 = (float)(1.0 - b2);
  for (int off = 0; off < n_segs; off += ADAMW_MAXSEG) {
    AdamwSegTable tb;
    tb.n = n_segs - off < ADAMW_MAXSEG ? n_segs - off : ADAMW_MAXSEG;
    int64_t want = 0;
    for (int i = 0; i < tb.n; ++i) want += (segs[off + i].end - segs[off + i].begin + 255) / 256;
    int grid = 0;
    for (int i = 0; i < tb.n; ++i) {
      const sow_adamw_segment& s = segs[off + i];
      const double bc1 = 1.0 - std::pow(b1, (double)s.step), bc2 = 1.0 - std::pow(b2, (double)s.step);
      AdamwSeg& d = tb.s[i];
      d.begin = s.begin, d.end = s.end;
      d.decay = (float)(1.0 - (double)s.lr * s.weight_decay), d.step_size = (float)(s.lr / bc1), d.bc2_sqrt = (float)std::sqrt(bc2);
      d.block0 = grid;
      // as launch_adamw_flat: one workgroup per 256 elements, the launch capped at 2048 (shared in proportion)
      int64_t nb = (s.end - s.begin + 255) / 256;
      if (want > 2048) nb = nb * 2048 / want;
      grid += nb < 1 ? 1 : (int)nb;
    }
    for (int i = tb.n; i < ADAMW_MAXSEG; ++i) tb.s[i] = AdamwSeg{0, 0, 1.f, 0.f, 1.f, grid};
#define SOW_ADAMW_SEG(T, TS) \
  hipLaunchKernelGGL((adamw_flat_seg_kernel<T, TS>), dim3(grid), dim3(256), 0, stream, (T*)p, (const T*)g, (TS*)m, (TS*)v, tb, b1f, c1, b2f, c2, eps, grad_scale)
    if (dtype == SOW_F32) SOW_ADAMW_SEG(float, float);
    else if (dtype == SOW_BF16 && state_dtype == SOW_BF16) SOW_ADAMW_SEG(bf16_t, bf16_t);
    else if (dtype == SOW_BF16) SOW_ADAMW_SEG(bf16_t, float);
    else if (state_dtype == SOW_F16) SOW_ADAMW_SEG(f16_t, f16_t);
    else SOW_ADAMW_SEG(f16_t, float);
#undef SOW_ADAMW_SEG
    SOW_CHECK_LAUNCH();
  }
  return SOW_OK;
}

// ---------------------------------------------------------------------------------------------
// The segment AdamW driven by a device record (sow_grad_stats, written by grad_stats.hip on the same stream before this
// launch): the gradient multiplier is stats->grad_mult instead of a host number, and with skip_nonfinite a record whose
// nonfinite flag is set makes every workgroup return before it touches p, m or v.  A segment may name a skip counter
// (device int32, the number of steps skipped so far, this one included): while it reads 0 -- or the segment names none --
// the three scalars are the host's, exactly adamw_flat_seg_kernel's, so with grad_mult == grad_scale the results are its
// bits; once it reads c > 0 one lane of the workgroup forms them for step max(1, step - c) in double from lr, weight_decay
// and the betas and rounds each once, as the host does.  Nobody writes the counters while this kernel reads them.
// ---------------------------------------------------------------------------------------------
struct AdamwStatSeg {
  int64_t begin, end;
  float decay, step_size, bc2_sqrt;
  int block0;   // first workgroup of this segment
  float lr, weight_decay;
  int step;
  int counter;  // index into skip_counters, -1: none
};
struct AdamwStatSegTable {
  AdamwStatSeg s[ADAMW_MAXSEG];
  int n;
};
static_assert(sizeof(AdamwStatSegTable) + 6 * sizeof(void*) + 2 * sizeof(double) + 5 * sizeof(float) + sizeof(int) <= 4096,
              "by-value kernel arguments must stay under 4 KiB");

template <typename T, typename TS>
__global__ __launch_bounds__(256) void adamw_flat_seg_stats_kernel(T* p, const T* g, TS* m, TS* v, const AdamwStatSegTable tb,
                                                                   float b1, float c1, float b2, float c2, float eps,
                                                                   double beta1, double beta2, const sow_grad_stats* stats,
                                                                   const int32_t* skip_counters, int skip_nonfinite) {
  if (skip_nonfinite && stats->nonfinite) return;   // uniform: the whole grid leaves
  const float grad_scale = stats->grad_mult;
  const int blk = blockIdx.x;
  int si = 0;
  while (si + 1 < tb.n && blk >= tb.s[si + 1].block0) ++si;   // uniform: scalar loads of the argument table
  const AdamwStatSeg& S = tb.s[si];
  const int nblk = (si + 1 < tb.n ? tb.s[si + 1].block0 : (int)gridDim.x) - S.block0;
  float decay = S.decay, step_size = S.step_size, bc2_sqrt = S.bc2_sqrt;
  const int skipped = S.counter >= 0 ? skip_counters[S.counter] : 0;
  if (skipped > 0) {   // uniform over the workgroup (one segment, one counter): lane 0 forms the scalars (the double pow, sqrt and
    // divide run in one wave of the four), LDS hands them on
    __shared__ float corrected[3];
    if (threadIdx.x == 0) {
      const int eff = S.step - skipped > 1 ? S.step - skipped : 1;
      const double bc1 = 1.0 - pow(beta1, (double)eff), bc2 = 1.0 - pow(beta2, (double)eff);
      corrected[0] = (float)(1.0 - (double)S.lr * S.weight_decay), corrected[1] = (float)(S.lr / bc1), corrected[2] = (float)sqrt(bc2);
    }
    __syncthreads();
    decay = corrected[0], step_size = corrected[1], bc2_sqrt = corrected[2];
  }
  const int64_t end = S.end, nth = (int64_t)nblk * blockDim.x;
  for (int64_t i = S.begin + (int64_t)(blk - S.block0) * blockDim.x + threadIdx.x; i < end; i += nth) {
    float pv = to_f32(p[i]);
    const float gv = to_f32(g[i]) * grad_scale;
    float mv = to_f32(m[i]), vv = to_f32(v[i]);
    pv *= decay;
    mv = b1 * mv + c1 * gv;
    vv = b2 * vv + c2 * gv * gv;
    const float denom = sqrtf(vv) / bc2_sqrt + eps;
    pv -= step_size * (mv / denom);
    p[i] = from_f32<T>(pv);
    m[i] = from_f32<TS>(mv);
    v[i] = from_f32<TS>(vv);
  }
}

int launch_adamw_flat_seg_stats(void* p, const void* g, void* m, void* v, const sow_adamw_segment* segs, const int* seg_counter,
                                int n_segs, double b1, double b2, float eps, const sow_grad_stats* stats, int skip_nonfinite,
                                const int32_t* skip_counters, int n_counters, int dtype, int state_dtype, hipStream_t stream) {
  if (n_segs < 0 || n_counters < 0) return SOW_ERR_SHAPE;
  if (!stats) return SOW_ERR_NULL;
  if (n_segs == 0) return SOW_OK;
  if (!p || !g || !m || !v || !segs || (n_counters > 0 && !skip_counters)) return SOW_ERR_NULL;
  const bool dt_ok = (dtype == SOW_F32 && state_dtype == SOW_F32) ||
                     ((dtype == SOW_BF16 || dtype == SOW_F16) && (state_dtype == dtype || state_dtype == SOW_F32));
  if (!dt_ok) return SOW_ERR_DTYPE;
  // every segment is checked before the first launch, by the rules of launch_adamw_flat_seg; a counter index is -1 or a
  // counter that exists
  for (int i = 0; i < n_segs; ++i) {
    if (segs[i].begin < 0 || segs[i].end <= segs[i].begin || segs[i].step < 1) return SOW_ERR_SHAPE;
    if (i && segs[i].begin < segs[i - 1].end) return SOW_ERR_SHAPE;
    if (seg_counter && (seg_counter[i] < -1 || seg_counter[i] >= n_counters)) return SOW_ERR_SHAPE;
  }
  const float b1f = (float)b1, c1 = (float)(1.0 - b1), b2f = (float)b2, c2 = (float)(1.0 - b2);
  for (int off = 0; off < n_segs; off += ADAMW_MAXSEG) {
    AdamwStatSegTable tb;
    tb.n = n_segs - off < ADAMW_MAXSEG ? n_segs - off : ADAMW_MAXSEG;
    int64_t want = 0;
    for (int i = 0; i < tb.n; ++i) want += (segs[off + i].end - segs[off + i].begin + 255) / 256;
    int grid = 0;
    for (int i = 0; i < tb.n; ++i) {
      const sow_adamw_segment& s = segs[off + i];
      const double bc1 = 1.0 - std::pow(b1, (double)s.step), bc2 = 1.0 - std::pow(b2, (double)s.step);
      AdamwStatSeg& d = tb.s[i];
      d.begin = s.begin, d.end = s.end;
      d.decay = (float)(1.0 - (double)s.lr * s.weight_decay), d.step_size = (float)(s.lr / bc1), d.bc2_sqrt = (float)std::sqrt(bc2);
      d.block0 = grid;
      d.lr = s.lr, d.weight_decay = s.weight_decay, d.step = s.step, d.counter = seg_counter ? seg_counter[off + i] : -1;
      // the grid of launch_adamw_flat_seg: one workgroup per 256 elements, the launch capped at 2048 (shared in proportion)
      int64_t nb = (s.end - s.begin + 255) / 256;
      if (want > 2048) nb = nb * 2048 / want;
      grid += nb < 1 ? 1 : (int)nb;
    }
    for (int i = tb.n; i < ADAMW_MAXSEG; ++i) tb.s[i] = AdamwStatSeg{0, 0, 1.f, 0.f, 1.f, grid, 0.f, 0.f, 1, -1};
#define SOW_ADAMW_SEG_STATS(T, TS) \
  hipLaunchKernelGGL((adamw_flat_seg_stats_kernel<T, TS>), dim3(grid), dim3(256), 0, stream, (T*)p, (const T*)g, (TS*)m, (TS*)v, tb, b1f, c1, b2f, c2, eps, b1, b2, stats, skip_counters, skip_nonfinite)
    if (dtype == SOW_F32) SOW_ADAMW_SEG_STATS(float, float);
    else if (dtype == SOW_BF16 && state_dtype == SOW_BF16) SOW_ADAMW_SEG_STATS(bf16_t, bf16_t);
    else if (dtype == SOW_BF16) SOW_ADAMW_SEG_STATS(bf16_t, float);
    else if (state_dtype == SOW_F16) SOW_ADAMW_SEG_STATS(f16_t, f16_t);
    else SOW_ADAMW_SEG_STATS(f16_t, float);
#undef SOW_ADAMW_SEG_STATS
    SOW_CHECK_LAUNCH();
  }
  return SOW_OK;
}

// ---------------------------------------------------------------------------------------------
// TTAdam dense section (ttadam.py:84-111), fp32:  v<0 -> 0 clamp (only when clamp_v), then
//   m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g*g ; p += -step_size * m/(sqrt(v)+eps) ; p += -lr*wd*p
// 1 - b is formed in double on the host from double betas (the Python-float alpha = 1.0 - beta of ttadam.py:91-92).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ttadam_dense_kernel(float* p, const float* g, float* m, float* v, int64_t n,
                                                           float b1, float c1, float b2, float c2, float eps,
                                                           float step_size, float lr_wd, int clamp_v) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = tid; i < n; i += nth) {
    const float gv = g[i];
    float vv = v[i];
    if (clamp_v && vv < 0.f) vv = 0.f;
    const float mv = m[i] * b1 + gv * c1;
    vv = vv * b2 + gv * gv * c2;
    float pv = p[i] + (mv / (sqrtf(vv) + eps)) * (-step_size);
    if (lr_wd > 0.f) pv = pv + pv * (-lr_wd);
    p[i] = pv;
    m[i] = mv;
    v[i] = vv;
  }
}

int launch_ttadam_dense(float* p, const float* g, float* m, float* v, int64_t n, double b1, double b2, float eps,
                        float step_size, float lr_wd, int clamp_v, hipStream_t stream) {
  if (n <= 0) return SOW_OK;
  if (!p || !g || !m || !v) return SOW_ERR_NULL;
  int grid = (int)((n + 255) / 256);
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL(ttadam_dense_kernel, dim3(grid), dim3(256), 0, stream, p, g, m, v, n, (float)b1, (float)(1.0 - b1),
                     (float)b2, (float)(1.0 - b2), eps, step_size, lr_wd, clamp_v);
  SOW_CHECK_LAUNCH();
  return SOW_OK;
}

// ---------------------------------------------------------------------------------------------
// TT Hadamard core product: out[(a,c), i, j, (b,d)] = A[a,i,j,b] * B[c,i,j,d]   (tt.py:469-475)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tt_kron_core_kernel(const float* A, const float* B, float* out, int ra0, int rb0,
                                                           int ij, int ra1, int rb1) {
  const int64_t n = (int64_t)ra0 * rb0 * ij * ra1 * rb1;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
  for (int64_t idx = tid; idx < n; idx += nth) {
    int64_t q = idx;
    const int d = (int)(q % rb1);
    q /= rb1;
    const int b = (int)(q % ra1);
    q /= ra1;
    const int e = (int)(q % ij);
    q /= ij;
    const int c = (int)(q % rb0);
    const int a = (int)(q / rb0);
    out[idx] = A[((int64_t)a * ij + e) * ra1 + b] * B[((int64_t)c * ij + e) * rb1 + d];
  }
}

int launch_tt_kron_core(const float* A, const float* B, float* out, int ra0, int rb0, int ij, int ra1, int rb1,
                        hipStream_t stream) {
  const int64_t n = (int64_t)ra0 * rb0 * ij * ra1 * rb1;
  if (n <= 0) return SOW_OK;
  if (!A || !B || !out) return SOW_ERR_NULL;
  int grid = (int)((n + 255) / 256);
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL(tt_kron_core_kernel, dim3(grid), dim3(256), 0, stream, A, B, out, ra0, rb0, ij, ra1, rb1);
  SOW_CHECK_LAUNCH();
  return SOW_OK;
}

// ---------------------------------------------------------------------------------------------
// max |x| over a contiguous fp32 buffer (TensorTrain.sqrt / sqrtinv scaling, tt.py:288, 322): one
// workgroup, result written to out[0]
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void absmax_kernel(const float* x, int64_t n, float* out) {
  __shared__ float red[16];
  float m = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += 1024) m = fmaxf(m, fabsf(x[i]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < 16; ++q) m = fmaxf(m, red[q]);
    out[0] = m;
  }
}

int launch_absmax(const float* x, int64_t n, float* out, hipStream_t stream) {
  if (!x || !out) return SOW_ERR_NULL;
  if (n < 0) return SOW_ERR_SHAPE;
  hipLaunchKernelGGL(absmax_kernel, dim3(1), dim3(1024), 0, stream, x, n, out);
  SOW_CHECK_LAUNCH();
  return SOW_OK;
}

// ---------------------------------------------------------------------------------------------
// Batched inverse of small [r, r] matrices by Gauss-Jordan with partial pivoting, one thread per matrix
// (TensorTrain.reciprocal, tt.py:480-494: the middle cores' [:, i, j, :] slices).  In [batch, r, r] fp32.
// ---------------------------------------------------------------------------------------------
constexpr int INV_MAX_R = 16;
__global__ __launch_bounds__(64) void small_inverse_kernel(const float* A, float* out, int batch, int r) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  float a[INV_MAX_R][INV_MAX_R], inv[INV_MAX_R][INV_MAX_R];
  for (int i = 0; i < r; ++i)
    for (int j = 0; j < r; ++j) {
      a[i][j] = A[((int64_t)b * r + i) * r + j];
      inv[i][j] = i == j ? 1.f : 0.f;
    }
  for (int c = 0; c < r; ++c) {
    int piv = c;
    float best = fabsf(a[c][c]);
    for (int i = c + 1; i < r; ++i)
      if (fabsf(a[i][c]) > best) best = fabsf(a[i][c]), piv = i;
    if (piv != c)
      for (int j = 0; j < r; ++j) {
        float t = a[c][j]; a[c][j] = a[piv][j]; a[piv][j] = t;
        t = inv[c][j]; inv[c][j] = inv[piv][j]; inv[piv][j] = t;
      }
    const float d = 1.f / a[c][c];
    for (int j = 0; j < r; ++j) a[c][j] *= d, inv[c][j] *= d;
    for (int i = 0; i < r; ++i) {
      if (i == c) continue;
      const float f = a[i][c];
      for (int j = 0; j < r; ++j) a[i][j] -= f * a[c][j], inv[i][j] -= f * inv[c][j];
    }
  }
  for (int i = 0; i < r; ++i)
    for (int j = 0; j < r; ++j) out[((int64_t)b * r + i) * r + j] = inv[i][j];
}

int launch_small_inverse(const float* A, float* out, int batch, int r, hipStream_t stream) {
  if (!A || !out) return SOW_ERR_NULL;
  if (batch < 0 || r < 1 || r > INV_MAX_R) return SOW_ERR_UNSUPPORTED;
  if (batch == 0) return SOW_OK;
  hipLaunchKernelGGL(small_inverse_kernel, dim3((batch + 63) / 64), dim3(64), 0, stream, A, out, batch, r);
  SOW_CHECK_LAUNCH();
  return SOW_OK;
}

// y = a*x + b*y   (fp32, bf16 or f16)
template <typename T>
__global__ __launch_bounds__(256) void axpby_kernel(const T* x, T* y, int64_t n, float a, float b) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = tid; i < n; i += nth) {
    const float yv = b != 0.f ? b * to_f32(y[i]) : 0.f;
    y[i] = from_f32<T>(a * to_f32(x[i]) + yv);
  }
}

int launch_axpby(const void* x, void* y, int64_t n, float a, float b, int dtype, hipStream_t stream) {
  if (n <= 0) return SOW_OK;
  if (!x || !y) return SOW_ERR_NULL;
  int grid = (int)((n + 255) / 256);
  if (grid > 2048) grid = 2048;
  if (dtype == SOW_F32)
    hipLaunchKernelGGL(axpby_kernel<float>, dim3(grid), dim3(256), 0, stream, (const float*)x, (float*)y, n, a, b);
  else if (dtype == SOW_BF16)
    hipLaunchKernelGGL(axpby_kernel<bf16_t>, dim3(grid), dim3(256), 0, stream, (const bf16_t*)x, (bf16_t*)y, n, a, b);
  else if (dtype == SOW_F16)
    hipLaunchKernelGGL(axpby_kernel<f16_t>, dim3(grid), dim3(256), 0, stream, (const f16_t*)x, (f16_t*)y, n, a, b);
  else
    return SOW_ERR_DTYPE;
  SOW_CHECK_LAUNCH();
  return SOW_OK;
}

// ---------------------------------------------------------------------------------------------
// Parameter pack (SOW_PARAM_F32): every fp32 parameter operand of a call -- A, B, bias, the accumulator, of every layer of a
// group -- rounded once, RNE, to the compute dtype in ONE launch; grid.y = tensor, grid.x = chunks of 8 elements per thread.
// from_f32<T> is the rounding the kernels apply to their own outputs, and torch's .to(bfloat16 / float16).
// ---------------------------------------------------------------------------------------------
constexpr int PK_MAX = 40;   // tensors per launch: 40 x 24 bytes of by-value arguments
struct PackTable {
  PackItem it[PK_MAX];
  int n;
};
static_assert(sizeof(PackTable) <= 4096, "by-value kernel arguments must stay under 4 KiB");

template <typename T> __global__ __launch_bounds__(256) void pack_params_kernel(const PackTable tb) {
  const int ti = blockIdx.y;
  if (ti >= tb.n) return;
  const float* src = tb.it[ti].src;
  T* dst = (T*)tb.it[ti].dst;
  const int64_t n = tb.it[ti].n;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
  int64_t done = 0;
  if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
    const int64_t nv = n / 8;
    for (int64_t i = tid; i < nv; i += nth) {
      const f32x4 a = *(const f32x4*)(src + 8 * i), b = *(const f32x4*)(src + 8 * i + 4);
      *(u32x4*)(dst + 8 * i) = u32x4{pack16x2<T>(a[0], a[1]), pack16x2<T>(a[2], a[3]), pack16x2<T>(b[0], b[1]),
                                     pack16x2<T>(b[2], b[3])};
    }
    done = nv * 8;
  }
  for (int64_t i = done + tid; i < n; i += nth) dst[i] = from_f32<T>(src[i]);
}

int launch_pack_params(const PackItem* items, int n, int dtype, hipStream_t stream) {
  if (dtype != SOW_BF16 && dtype != SOW_F16) return SOW_ERR_DTYPE;
  for (int off = 0; off < n; off += PK_MAX) {
    PackTable tb;
    tb.n = n - off < PK_MAX ? n - off : PK_MAX;
    int64_t maxn = 0;
    for (int i = 0; i < tb.n; ++i) {
      tb.it[i] = items[off + i];
      if (tb.it[i].n < 0) return SOW_ERR_SHAPE;
      if (tb.it[i].n > 0 && (!tb.it[i].src || !tb.it[i].dst)) return SOW_ERR_NULL;
      if (tb.it[i].n > maxn) maxn = tb.it[i].n;
    }
    if (maxn == 0) continue;
    int64_t gx = (maxn / 8 + 255) / 256;
    if (gx < 1) gx = 1;
    if (gx > 256) gx = 256;
    if (dtype == SOW_BF16)
      hipLaunchKernelGGL(pack_params_kernel<bf16_t>, dim3((unsigned)gx, tb.n), dim3(256), 0, stream, tb);
    else
      hipLaunchKernelGGL(pack_params_kernel<f16_t>, dim3((unsigned)gx, tb.n), dim3(256), 0, stream, tb);
    SOW_CHECK_LAUNCH();
  }
  return SOW_OK;
}

}  // namespace sow
