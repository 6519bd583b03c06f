// Householder QR of a column panel, LAPACK conventions (geqr2 + org2r), fp32 internals.
//
// Reference call sites: tn_gradient/utils.py:8-30 (qr_weight: reduced QR, keep Q[:, :k], R[:k, :]),
// tn_gradient/layer/sow.py:96-99 (init), :144-150 (truncated QR of the accumulator), :168-172 (A re-init
// keeps only Q[:, :r] of an [in, out] Gaussian), tn_gradient/tt.py:128-136 (complete-mode QR, truncated).
// Only the first kc = min(k, m, n) columns have to be factored to obtain Q[:, :k]; R[:k, j] for j >= kc
// is Q[:, :k]^T W[:, j], computed by the GEMM kernel from the host wrapper in api.hip.
//
// Sign convention (LAPACK slarfg): beta = -sign(alpha) * ||x||, tau = (beta - alpha) / beta,
// v = x / (alpha - beta), v[0] = 1;  a zero sub-column gives tau = 0 (H = I).  diag(R) therefore has
// mixed signs exactly as torch.linalg.qr on CPU.
//
// One workgroup (1024 threads = 16 waves) per matrix: the panel lives column-major in a global fp32
// workspace (L2 resident), the active reflector is cached in LDS, every wave owns trailing columns
// (dot product + rank-1 update with wave-64 shuffles), two workgroup barriers per column.
#include "kernels.hpp"
#include "qr_panel.hpp"

namespace sow {

__global__ __launch_bounds__(QR_THREADS) void qr_panel_kernel(float* Pt, float* Qt, int m, int kc, int r) {
  extern __shared__ __attribute__((aligned(16))) float qsm[];
  qr_panel_body(Pt, Qt, m, kc, r, qsm);
}

// Qt [r][m] fp32 -> Q [m, r] row-major Tout ; upper triangle of the factored panel -> R[:k, :kc]
template <typename Tout>
__global__ void qr_copy_out_kernel(const float* Qt, const float* Pt, Tout* Q, int64_t ldq, Tout* R, int64_t ldr, int m,
                                   int kc, int r, int k_rows) {
  const int64_t nq = (int64_t)m * r;
  const int64_t nr = R ? (int64_t)k_rows * kc : 0;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < nq + nr;
       idx += (int64_t)gridDim.x * blockDim.x) {
    if (idx < nq) {
      const int i = (int)(idx / r), c = (int)(idx % r);
      Q[(int64_t)i * ldq + c] = from_f32<Tout>(Qt[(int64_t)c * m + i]);
    } else {
      const int64_t e = idx - nq;
      const int i = (int)(e / kc), c = (int)(e % kc);
      const float v = (i <= c && i < m) ? Pt[(int64_t)c * m + i] : 0.f;
      R[(int64_t)i * ldr + c] = from_f32<Tout>(v);
    }
  }
}

// generic 2-D cast copy (strided rows), used for the fp32 staging of bf16 inputs / outputs
template <typename Tin, typename Tout>
__global__ void cast_copy_kernel(const Tin* src, int64_t lds, Tout* dst, int64_t ldd, int64_t rows, int cols) {
  const int64_t n = rows * cols;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = idx / cols;
    const int c = (int)(idx % cols);
    dst[i * ldd + c] = from_f32<Tout>(to_f32(src[i * lds + c]));
  }
}

// contiguous, 16-byte aligned casts (the fp32 x of a layer under autocast and its gradient): 8 elements per thread, 16-byte
// accesses on the 16-bit side
template <typename Tin, typename Tout> __device__ __forceinline__ void cast8(const Tin* s, Tout* d) {
  Tin v[8];
  Tout o[8];
  if constexpr (sizeof(Tin) == 4) {
    *(f32x4*)v = *(const f32x4*)s;
    *(f32x4*)(v + 4) = *(const f32x4*)(s + 4);
  } else {
    *(u32x4*)v = *(const u32x4*)s;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = from_f32<Tout>(to_f32(v[j]));
  if constexpr (sizeof(Tout) == 4) {
    *(f32x4*)d = *(const f32x4*)o;
    *(f32x4*)(d + 4) = *(const f32x4*)(o + 4);
  } else {
    *(u32x4*)d = *(const u32x4*)o;
  }
}
template <typename Tin, typename Tout> __global__ __launch_bounds__(256) void cast_flat_kernel(const Tin* src, Tout* dst, int64_t n) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
  const int64_t nv = n / 8;
  for (int64_t i = tid; i < nv; i += nth) cast8(src + 8 * i, dst + 8 * i);
  for (int64_t i = nv * 8 + tid; i < n; i += nth) dst[i] = from_f32<Tout>(to_f32(src[i]));
}

static int grid_for(int64_t n) {
  int64_t g = (n + 255) / 256;
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  return (int)g;
}

// The image of an E4M3 accumulator: dst[k][n] = e4m3(q[k][n]) * 2^exps[n], codes [d_in][d_out] row-major, one byte each.  A
// thread takes 8 columns of a row: an 8-byte load of codes (each read once), an 8-byte load of exponents, the hardware
// conversion, the scaling in fp32 (v_ldexp_f32, exact: |e| <= 119) and a conversion that rounds nothing (the product is a number of
// Tout by the format's contract), one 16-byte store.  The two NaN codes give NaN.
template <typename Tout>
__global__ __launch_bounds__(256) void cast_copy_kernel(const uint8_t* q, const int8_t* exps, Tout* dst, int64_t ldd, int d_in, int d_out) {
  typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
  const int nv = d_out / 8;
  const int64_t n = (int64_t)d_in * nv;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = idx / nv;
    const int c = (int)(idx - k * nv) * 8;
    const u32x2 qv = *(const u32x2*)(q + k * d_out + c);
    const u32x2 ev = *(const u32x2*)(exps + c);
    Tout o[8];
#pragma unroll
    for (int wd = 0; wd < 2; ++wd) {
      const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8(qv[wd], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(qv[wd], true);
      const float v[4] = {lo[0], lo[1], hi[0], hi[1]};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e = (int)(int8_t)(ev[wd] >> (8 * j));
        o[4 * wd + j] = from_f32<Tout>(__builtin_ldexpf(v[j], e));   // (not a multiply: fused into the f16 conversion it loses -0)
      }
    }
    *(u32x4*)(dst + k * ldd + c) = *(const u32x4*)o;
  }
}

int launch_acc_dequantize(const void* q, const void* exps, int d_in, int d_out, void* dst, int64_t ldd, int dst_dtype,
                          hipStream_t stream) {
  if (dst_dtype != SOW_BF16 && dst_dtype != SOW_F16) return SOW_ERR_DTYPE;
  const int g = grid_for((int64_t)d_in * (d_out / 8));
  if (dst_dtype == SOW_BF16)
    hipLaunchKernelGGL((cast_copy_kernel<bf16_t>), dim3(g), dim3(256), 0, stream, (const uint8_t*)q, (const int8_t*)exps,
                       (bf16_t*)dst, ldd, d_in, d_out);
  else
    hipLaunchKernelGGL((cast_copy_kernel<f16_t>), dim3(g), dim3(256), 0, stream, (const uint8_t*)q, (const int8_t*)exps,
                       (f16_t*)dst, ldd, d_in, d_out);
  SOW_CHECK_LAUNCH();
  return SOW_OK;
}

// The image of an MXFP4 accumulator: dst[k][n] = e2m1(code(k, n)) * 2^(scales[k / 32][n] - 127), codes [d_in / 2][d_out], one
// byte = rows k (low nibble) and k + 1 of a column, scales [d_in / 32][d_out] E8M0 bytes.  A thread takes 8 columns of a row
// pair: an 8-byte load of codes (each read once), an 8-byte load of scale bytes, eight scaled conversions (each a pair of Tout:
// the two rows of one column, exact, -0 kept), regrouped into the two rows: two 16-byte stores.
template <typename Tout>
__global__ __launch_bounds__(256) void cast_copy_kernel(const uint8_t* q, const uint8_t* scales, Tout* dst, int64_t ldd, int d_in, int d_out) {
  const int nv = d_out / 8;
  const int64_t n = (int64_t)(d_in / 2) * nv;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t kp = idx / nv;
    const int c = (int)(idx - kp * nv) * 8;
    const u32x2 qv = *(const u32x2*)(q + kp * d_out + c);
    const u32x2 sv = *(const u32x2*)(scales + (kp >> 4) * d_out + c);
    uint32_t pr[8];   // column j: row 2 kp in the low half, row 2 kp + 1 in the high half
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float sc = __uint_as_float(((sv[j >> 2] >> (8 * (j & 3))) & 0xffu) << 23);
      pr[j] = cvt_fp4_pair<Tout>(qv[j >> 2], sc, j & 3);
    }
    u32x4 r0, r1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      r0[j] = __builtin_amdgcn_perm(pr[2 * j + 1], pr[2 * j], 0x05040100u);
      r1[j] = __builtin_amdgcn_perm(pr[2 * j + 1], pr[2 * j], 0x07060302u);
    }
    Tout* d = dst + 2 * kp * ldd + c;
    *(u32x4*)d = r0;
    *(u32x4*)(d + ldd) = r1;
  }
}

int launch_acc_dequantize_fp4(const void* q, const void* scales, int d_in, int d_out, void* dst, int64_t ldd, int dst_dtype,
                              hipStream_t stream) {
  if (dst_dtype != SOW_BF16 && dst_dtype != SOW_F16) return SOW_ERR_DTYPE;
  const int g = grid_for((int64_t)(d_in / 2) * (d_out / 8));
  if (dst_dtype == SOW_BF16)
    hipLaunchKernelGGL((cast_copy_kernel<bf16_t>), dim3(g), dim3(256), 0, stream, (const uint8_t*)q, (const uint8_t*)scales,
                       (bf16_t*)dst, ldd, d_in, d_out);
  else
    hipLaunchKernelGGL((cast_copy_kernel<f16_t>), dim3(g), dim3(256), 0, stream, (const uint8_t*)q, (const uint8_t*)scales,
                       (f16_t*)dst, ldd, d_in, d_out);
  SOW_CHECK_LAUNCH();
  return SOW_OK;
}

int launch_cast_copy(const void* src, int64_t lds, int src_dtype, void* dst, int64_t ldd, int dst_dtype, int64_t rows,
                     int cols, hipStream_t stream) {
  if (rows <= 0 || cols <= 0) return SOW_OK;
  const bool flat = (rows == 1 || (lds == cols && ldd == cols)) &&
                    ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
  const int g = grid_for(flat ? (rows * cols + 7) / 8 : rows * cols);
#define SOW_CAST(Tin, Tout)                                                                                                   \
  do {                                                                                                                      \
    if (flat)                                                                                                               \
      hipLaunchKernelGGL((cast_flat_kernel<Tin, Tout>), dim3(g), dim3(256), 0, stream, (const Tin*)src, (Tout*)dst, rows * cols); \
    else                                                                                                                    \
      hipLaunchKernelGGL((cast_copy_kernel<Tin, Tout>), dim3(g), dim3(256), 0, stream, (const Tin*)src, lds, (Tout*)dst, ldd, \
                         rows, cols);                                                                                       \
  } while (0)
#define SOW_CAST_TO(Tin)                                     \
  if (dst_dtype == SOW_F32) SOW_CAST(Tin, float);            \
  else if (dst_dtype == SOW_BF16) SOW_CAST(Tin, bf16_t);     \
  else if (dst_dtype == SOW_F16) SOW_CAST(Tin, f16_t);       \
  else return SOW_ERR_DTYPE;
  if (src_dtype == SOW_F32) {
    SOW_CAST_TO(float)
  } else if (src_dtype == SOW_BF16) {
    SOW_CAST_TO(bf16_t)
  } else if (src_dtype == SOW_F16) {
    SOW_CAST_TO(f16_t)
  } else
    return SOW_ERR_DTYPE;
#undef SOW_CAST_TO
#undef SOW_CAST
  SOW_CHECK_LAUNCH();
  return SOW_OK;
}

size_t qr_panel_lds_bytes(int m, int kc) { return ((size_t)m + kc + 16) * sizeof(float); }

// Factor W[:, :kc] and form Q[:, :r].  Pt: [kc*m] floats, Qt: [r*m] floats (workspace).
int launch_qr_panel(const void* W, int64_t ldw, int in_dtype, int m, int kc, int r, float* Pt, float* Qt,
                    hipStream_t stream) {
  if (m <= 0 || kc <= 0 || r <= 0 || kc > m || r > m) return SOW_ERR_SHAPE;
  const size_t lds = qr_panel_lds_bytes(m, kc);
  if (lds > 150 * 1024) return SOW_ERR_UNSUPPORTED;
  const int g = grid_for((int64_t)m * kc);
  if (in_dtype == SOW_F32)
    hipLaunchKernelGGL(qr_copy_in_kernel<float>, dim3(g), dim3(256), 0, stream, (const float*)W, ldw, Pt, m, kc);
  else if (in_dtype == SOW_BF16)
    hipLaunchKernelGGL(qr_copy_in_kernel<bf16_t>, dim3(g), dim3(256), 0, stream, (const bf16_t*)W, ldw, Pt, m, kc);
  else if (in_dtype == SOW_F16)
    hipLaunchKernelGGL(qr_copy_in_kernel<f16_t>, dim3(g), dim3(256), 0, stream, (const f16_t*)W, ldw, Pt, m, kc);
  else
    return SOW_ERR_DTYPE;
  SOW_CHECK_LAUNCH();
  SOW_SET_MAX_LDS_ONCE(150 * 1024, qr_panel_kernel);
  hipLaunchKernelGGL(qr_panel_kernel, dim3(1), dim3(QR_THREADS), lds, stream, Pt, Qt, m, kc, r);
  SOW_CHECK_LAUNCH();
  return SOW_OK;
}

int launch_qr_copy_out(const float* Qt, const float* Pt, void* Q, int64_t ldq, void* R, int64_t ldr, int out_dtype, int m,
                       int kc, int r, int k_rows, hipStream_t stream) {
  const int g = grid_for((int64_t)m * r + (R ? (int64_t)k_rows * kc : 0));
  if (out_dtype == SOW_F32)
    hipLaunchKernelGGL(qr_copy_out_kernel<float>, dim3(g), dim3(256), 0, stream, Qt, Pt, (float*)Q, ldq, (float*)R, ldr, m, kc, r, k_rows);
  else if (out_dtype == SOW_BF16)
    hipLaunchKernelGGL(qr_copy_out_kernel<bf16_t>, dim3(g), dim3(256), 0, stream, Qt, Pt, (bf16_t*)Q, ldq, (bf16_t*)R, ldr, m, kc, r, k_rows);
  else if (out_dtype == SOW_F16)
    hipLaunchKernelGGL(qr_copy_out_kernel<f16_t>, dim3(g), dim3(256), 0, stream, Qt, Pt, (f16_t*)Q, ldq, (f16_t*)R, ldr, m, kc, r, k_rows);
  else
    return SOW_ERR_DTYPE;
  SOW_CHECK_LAUNCH();
  return SOW_OK;
}

}  // namespace sow
