// Weight gradients of a wide-rank layer (64 < r <= 256, bf16 / f16), split over token slabs so that the grid fills the chip:
//
//   dA    = x^T . dh            [d_in, r]
//   dB    = scale * h^T . dY    [r, d_out]    (h_save is the unscaled x . A for r > 64)
//   dbias = sum_t dY            [d_out]       (side sum of the dY tiles the kernel streams anyway: no extra pass over dY)
//
// The generic composition runs the two products as transposed 128 x 128-tile GEMMs with K = T: at d = 2048, r = 200 that is
// 32 workgroups per product, each streaming every token.  Here a workgroup owns 64 columns of x (or dY) and all r_pad
// columns of dh (or h) for one token slab, and writes an fp32 partial [64][r_pad] to the workspace; tnw_reduce_kernel sums
// the slabs in a fixed order (slab 0, 1, ...) -- no atomics, bit-identical from run to run.
//
// Operands are stored token-major (the contraction index is the row index), so both are staged as dword pairs of 8
// consecutive tokens and transposed in registers (transpose_8x2) into k-contiguous LDS images, as the generic GEMM does
// for a transposed operand.  LDS: M image [64][64] 8 KiB, S image [256][64] 32 KiB.
//
// Ragged widths (RAG: d_in or d_out not a multiple of 8): a row of x / dY starts at any 2-byte offset, so the column pair
// of an M item is read as two 16-bit loads (each column < D, nothing past a row or the tensor); the LDS images and the
// products are those of the aligned kernel.
#include "kernels.hpp"

namespace sow {

template <typename T, bool RAG>
__global__ __launch_bounds__(256, 2) void tnw_partial_kernel(const TnwParams p) {
  using V8 = typename DT<T>::v8;
  __shared__ __attribute__((aligned(16))) char mimg[64 * 64 * 2];
  __shared__ __attribute__((aligned(16))) char simg[256 * 64 * 2];
  __shared__ float red[8][64];

  const int t = threadIdx.x, lane = t & 63, w = t >> 6, li = lane & 31, lh = lane >> 5;
  const int ncg = p.ncg[0] + p.ncg[1];
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int s = lid / ncg;
  const int g = lid % ncg;
  const int job = g >= p.ncg[0] ? 1 : 0;
  const int d0 = (g - (job ? p.ncg[0] : 0)) * 64;
  const T* M = (const T*)p.M[job];
  const T* S = (const T*)p.S[job];
  const int D = p.D[job], r = p.r, r_pad = p.r_pad, ntiles = 2 * (r_pad / 32);
  const int64_t tb = (int64_t)s * p.slab_len;
  const int64_t te = tb + p.slab_len < p.T ? tb + p.slab_len : p.T;
  const bool colsum = job == 1 && p.colsum != nullptr;

  f32x16 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
  float cs0 = 0.f, cs1 = 0.f;

  // M item: column pair mrp of the 64 columns, token octet mko;  S items: column pair rp = item & 127, octet item >> 7
  const int mrp = t & 31, mko = t >> 5;
  const bool mcol = d0 + 2 * mrp < D;
  uint32_t md[8], sd[4][8];
  auto load = [&](int64_t k0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int64_t gt = k0 + mko * 8 + j;
      if constexpr (RAG) {
        const unsigned short* m16 = (const unsigned short*)(M + gt * D + d0 + 2 * mrp);
        const uint32_t lo = (mcol && gt < te) ? m16[0] : 0u;
        const uint32_t hi = (d0 + 2 * mrp + 1 < D && gt < te) ? m16[1] : 0u;
        md[j] = lo | (hi << 16);
      } else {
        md[j] = (mcol && gt < te) ? *(const uint32_t*)(M + gt * D + d0 + 2 * mrp) : 0u;
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int item = t + 256 * q, c = 2 * (item & 127), ko = item >> 7;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int64_t gt = k0 + ko * 8 + j;
        sd[q][j] = (c < r && gt < te) ? *(const uint32_t*)(S + gt * r + c) : 0u;
      }
    }
  };
  load(tb);
  for (int64_t k0 = tb; k0 < te; k0 += 64) {
    __syncthreads();
    {
      u32x4 c0, c1;
      transpose_8x2(md, c0, c1);
      *(u32x4*)(mimg + bf16_img_off<64>(2 * mrp, mko)) = c0;
      *(u32x4*)(mimg + bf16_img_off<64>(2 * mrp + 1, mko)) = c1;
      if (colsum) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const T* e = (const T*)&md[j];
          cs0 += to_f32(e[0]);
          cs1 += to_f32(e[1]);
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int item = t + 256 * q, rp = item & 127, ko = item >> 7;
        if (2 * rp < r_pad) {
          transpose_8x2(sd[q], c0, c1);
          *(u32x4*)(simg + bf16_img_off<64>(2 * rp, ko)) = c0;
          *(u32x4*)(simg + bf16_img_off<64>(2 * rp + 1, ko)) = c1;
        }
      }
    }
    __syncthreads();
    if (k0 + 64 < te) load(k0 + 64);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const V8 a0 = *(const V8*)(mimg + bf16_img_off<64>(li, 2 * ks + lh));
      const V8 a1 = *(const V8*)(mimg + bf16_img_off<64>(32 + li, 2 * ks + lh));
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = w + 4 * i;
        if (j < ntiles) {
          const V8 b = *(const V8*)(simg + bf16_img_off<64>((j >> 1) * 32 + li, 2 * ks + lh));
          acc[i] = mfma32((j & 1) ? a1 : a0, b, acc[i]);
        }
      }
    }
  }

  // partial[s][d][c], d over the job's 64-column groups (Dpad rows), c < r_pad
  const int Dpad = p.ncg[job] * 64;
  float* P = p.partial[job] + (int64_t)s * Dpad * r_pad;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = w + 4 * i;
    if (j < ntiles) {
      const int c = (j >> 1) * 32 + li;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) P[(int64_t)(d0 + (j & 1) * 32 + acc_row(reg, lane)) * r_pad + c] = acc[i][reg];
    }
  }
  if (colsum) {
    red[mko][2 * mrp] = cs0;
    red[mko][2 * mrp + 1] = cs1;
    __syncthreads();
    if (t < 64) {
      float v = red[0][t];
#pragma unroll
      for (int k = 1; k < 8; ++k) v += red[k][t];
      p.colsum[(int64_t)s * Dpad + d0 + t] = v;
    }
  }
}

// One thread per output element: dA [d_in][r], then dB [r][d_out] (stored transposed w.r.t. the partials), then dbias.
template <typename T> __global__ __launch_bounds__(256) void tnw_reduce_kernel(const TnwReduce p) {
  const int64_t n0 = (int64_t)p.D0 * p.r, n1 = (int64_t)p.D1 * p.r;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int Dp0 = (p.D0 + 63) / 64 * 64, Dp1 = (p.D1 + 63) / 64 * 64;
  float v = 0.f;
  T* dst;
  float alpha = 1.f;
  if (i < n0) {
    const int d = (int)(i / p.r), c = (int)(i % p.r);
    for (int s = 0; s < p.ns; ++s) v += p.P0[((int64_t)s * Dp0 + d) * p.r_pad + c];
    dst = (T*)p.dA + i;
  } else if ((i -= n0) < n1) {
    const int d = (int)(i / p.r), c = (int)(i % p.r);
    for (int s = 0; s < p.ns; ++s) v += p.P1[((int64_t)s * Dp1 + d) * p.r_pad + c];
    dst = (T*)p.dB + (int64_t)c * p.D1 + d;
    alpha = p.scale;
  } else if ((i -= n1) < (p.dbias ? p.D1 : 0)) {
    for (int s = 0; s < p.ns; ++s) v += p.CS[(int64_t)s * Dp1 + i];
    dst = (T*)p.dbias + i;
  } else {
    return;
  }
  v *= alpha;
  if (p.beta != 0.f) v += p.beta * to_f32(*dst);
  *dst = from_f32<T>(v);
}

bool tnw_shape_ok(int r, int d_in, int d_out, int dtype) {
  return (dtype == SOW_BF16 || dtype == SOW_F16) && r > 64 && r <= 256 && r % 2 == 0 && d_in % 8 == 0 && d_out % 8 == 0;
}

// slab count: about two resident workgroups per CU (512), slabs of at least 256 tokens, a multiple of 64 long
int tnw_pick_slabs(int64_t T, int d_in, int d_out, int* slab_len) {
  const int tiles = (d_in + 63) / 64 + (d_out + 63) / 64;
  int64_t ns = (512 + tiles - 1) / tiles;
  const int64_t by_len = T / 256 > 0 ? T / 256 : 1;
  if (ns > by_len) ns = by_len;
  if (ns > 64) ns = 64;
  if (ns < 1) ns = 1;
  int64_t len = (T + ns - 1) / ns;
  len = (len + 63) / 64 * 64;
  if (len < 64) len = 64;
  *slab_len = (int)len;
  return (int)((T + len - 1) / len);
}

size_t tnw_partial_bytes(int64_t T, int d_in, int d_out, int r) {
  int len;
  const size_t ns = (size_t)tnw_pick_slabs(T, d_in, d_out, &len);
  const size_t r_pad = (size_t)(r + 63) / 64 * 64, dp0 = (size_t)(d_in + 63) / 64 * 64, dp1 = (size_t)(d_out + 63) / 64 * 64;
  return ((ns * dp0 * r_pad * 4 + 255) & ~(size_t)255) + ((ns * dp1 * r_pad * 4 + 255) & ~(size_t)255) +
         ((ns * dp1 * 4 + 255) & ~(size_t)255);
}

bool tnw_operands_ok(const void* x, const void* dh, const void* dy, const void* h, bool rag) {
  return (rag || (al4p(x) && al4p(dy))) && al4p(h) && al4p(dh);
}

int launch_tn_wide(const void* x, const void* dh, const void* dy, const void* h, void* dA, void* dB, void* dbias, int64_t T,
                   int d_in, int d_out, int r, float scale, float beta, int dtype, int out_dtype, void* ws, size_t ws_bytes,
                   hipStream_t stream) {
  // ragged widths: x and dY at any 2-byte offset (16-bit loads)
  const bool rag = d_in % 8 != 0 || d_out % 8 != 0;
  if (!(rag ? ragged_shape_ok(r, d_in, d_out, dtype) && r > 64 : tnw_shape_ok(r, d_in, d_out, dtype))) return SOW_ERR_UNSUPPORTED;
  if (out_dtype != dtype && out_dtype != SOW_F32) return SOW_ERR_DTYPE;
  if (!tnw_operands_ok(x, dh, dy, h, rag) || !ws || (reinterpret_cast<uintptr_t>(ws) & 255) ||
      ws_bytes < tnw_partial_bytes(T, d_in, d_out, r))
    return SOW_ERR_UNSUPPORTED;
  if (T <= 0) return SOW_ERR_SHAPE;
  TnwParams p{};
  const int ns = tnw_pick_slabs(T, d_in, d_out, &p.slab_len);
  const size_t r_pad = (size_t)(r + 63) / 64 * 64, dp0 = (size_t)(d_in + 63) / 64 * 64, dp1 = (size_t)(d_out + 63) / 64 * 64;
  char* base = (char*)ws;
  float* P0 = (float*)base;
  float* P1 = (float*)(base + ((ns * dp0 * r_pad * 4 + 255) & ~(size_t)255));
  float* CS = (float*)((char*)P1 + ((ns * dp1 * r_pad * 4 + 255) & ~(size_t)255));
  p.M[0] = x, p.S[0] = dh, p.partial[0] = P0, p.D[0] = d_in, p.ncg[0] = (d_in + 63) / 64;
  p.M[1] = dy, p.S[1] = h, p.partial[1] = P1, p.D[1] = d_out, p.ncg[1] = (d_out + 63) / 64;
  p.colsum = dbias ? CS : nullptr;
  p.T = T, p.r = r, p.r_pad = (int)r_pad, p.ns = ns;
  TnwReduce q{};
  q.P0 = P0, q.P1 = P1, q.CS = CS, q.dA = dA, q.dB = dB, q.dbias = dbias;
  q.D0 = d_in, q.D1 = d_out, q.r = r, q.r_pad = (int)r_pad, q.ns = ns, q.scale = scale, q.beta = beta;
  const int64_t blocks = (int64_t)ns * (p.ncg[0] + p.ncg[1]);
  const int64_t nout = (int64_t)(d_in + d_out) * r + (dbias ? d_out : 0);
  const dim3 pgrid((unsigned)blocks);
  if (dtype == SOW_BF16 && rag)
    hipLaunchKernelGGL((tnw_partial_kernel<bf16_t, true>), pgrid, dim3(256), 0, stream, p);
  else if (dtype == SOW_BF16)
    hipLaunchKernelGGL((tnw_partial_kernel<bf16_t, false>), pgrid, dim3(256), 0, stream, p);
  else if (rag)
    hipLaunchKernelGGL((tnw_partial_kernel<f16_t, true>), pgrid, dim3(256), 0, stream, p);
  else
    hipLaunchKernelGGL((tnw_partial_kernel<f16_t, false>), pgrid, dim3(256), 0, stream, p);
  // the reduction reads fp32 partials only: its template type is the type of the gradients it writes
  const dim3 rgrid((unsigned)((nout + 255) / 256));
  if (out_dtype == SOW_F32)
    hipLaunchKernelGGL(tnw_reduce_kernel<float>, rgrid, dim3(256), 0, stream, q);
  else if (dtype == SOW_BF16)
    hipLaunchKernelGGL(tnw_reduce_kernel<bf16_t>, rgrid, dim3(256), 0, stream, q);
  else
    hipLaunchKernelGGL(tnw_reduce_kernel<f16_t>, rgrid, dim3(256), 0, stream, q);
  SOW_CHECK_LAUNCH();
  return SOW_OK;
}

}  // namespace sow
