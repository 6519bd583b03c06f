// Blocked Householder QR (compact WY: LAPACK geqrt / larfb / orgqr structure) for panels wider than 64 columns.
//
// The unblocked panel of qr_panel.hpp runs the whole factorisation on one workgroup.  Here only a block of QRB_NB columns is
// factored that way (qr_block_panel_kernel: the same slarfg arithmetic, signs and taus as qr_panel_body, on rows j0.. of
// columns j0 .. j0 + jb), followed by the block's triangular factor T (H_0 .. H_{jb-1} = I - V T V^T, slarft forward /
// columnwise), and the rest of the chip applies the block reflector to the trailing columns:
//
//   factorisation, block by block:   C <- (I - V T^T V^T) C   on Pt columns j0 + jb .. kc
//   Q = H_0 .. H_{kc-1} I[:, :r]:    C <- (I - V T V^T) C     on Qt columns j0 .. r, blocks in reverse order
//
// qr_larfb_kernel: one 512-thread workgroup per QRB_NC columns of C.  Phase 1 forms W = V^T C (wave w owns the reflector
// columns w, w + 8, ..; lanes stride over the rows; one shuffle reduction per W element), phase 2 W <- op(T) W from LDS, phase 3
// C -= V W (a thread owns rows, all QRB_NC columns).  V and C are column-major, so every wave access is a contiguous run of
// rows; the columns of one workgroup stay in L2 between phase 1 and phase 3, V ((m - j0) x jb floats) is L2 resident for the
// whole step.  fp32 FMAs only, every reduction in a fixed order, no atomics: results repeat bit for bit.
//
// V is unit lower trapezoidal and shares its storage with R: entries on and above the diagonal of the block are read as 1 / 0,
// never from memory's values.  T is written in full (zeros below the diagonal and past a partial block), one QRB_NB x QRB_NB
// tile per block, kept for the Q phase.
#include "kernels.hpp"
#include "qr_panel.hpp"

namespace sow {

#ifndef SOW_QR_NB
#define SOW_QR_NB 32
#endif
constexpr int QRB_NB = SOW_QR_NB;   // block width: 32 or 64 (profiles/qr_blocked.txt)
constexpr int QRB_NC = 8;           // columns of C per workgroup
constexpr int QRB_THREADS = 512;
constexpr int QRB_WAVES = QRB_THREADS / 64;
static_assert(QRB_NB == 32 || QRB_NB == 64, "block width");
static_assert(QRB_NB * QRB_NC <= QRB_THREADS && QRB_NB % QRB_WAVES == 0 && QRB_NB <= 64, "larfb thread layout");

size_t qr_blocked_t_floats(int kc) { return (size_t)ceil_div(kc, QRB_NB) * QRB_NB * QRB_NB; }

// dynamic LDS: max(m - j0, NB * NB) floats (the active reflector during the panel, V^T V afterwards)
__global__ __launch_bounds__(QR_THREADS) void qr_block_panel_kernel(float* Pt, float* T, int m, int j0, int jb) {
  constexpr int NB = QRB_NB;
  extern __shared__ __attribute__((aligned(16))) float qsm[];
  __shared__ float taus[NB], red[QR_THREADS / 64];
  __shared__ float sh_tau;
  float* vs = qsm;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int mr = m - j0;
  float* P = Pt + (int64_t)j0 * m + j0;   // P[c * m + i]: row j0 + i of column j0 + c

  for (int j = 0; j < jb; ++j) {
    float* col = P + (int64_t)j * m;
    float s = 0.f;
    for (int i = j + 1 + tid; i < mr; i += QR_THREADS) {
      const float a = col[i];
      s += a * a;
    }
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    if (tid == 0) {
      float x2 = 0.f;
      for (int q = 0; q < QR_THREADS / 64; ++q) x2 += red[q];
      const float alpha = col[j];
      float tau = 0.f, scale = 0.f;
      if (x2 != 0.f) {
        const float nrm = sqrtf(alpha * alpha + x2);
        const float beta = alpha >= 0.f ? -nrm : nrm;  // -sign(alpha) * nrm, sign(0) = +
        tau = (beta - alpha) / beta;
        scale = 1.f / (alpha - beta);
        col[j] = beta;
      }
      taus[j] = tau;
      sh_tau = tau;
      red[0] = scale;
    }
    __syncthreads();
    const float tau = sh_tau, scale = red[0];
    for (int i = j + tid; i < mr; i += QR_THREADS) {
      if (i == j) {
        vs[i] = 1.f;
      } else {
        const float v = col[i] * scale;
        col[i] = v;
        vs[i] = v;
      }
    }
    __syncthreads();
    if (tau != 0.f) {
      for (int c = j + 1 + wave; c < jb; c += QR_THREADS / 64) {
        float* cc = P + (int64_t)c * m;
        float d = 0.f;
#pragma unroll 4
        for (int i = j + lane; i < mr; i += 64) d += vs[i] * cc[i];
        d = wave_sum(d) * tau;
#pragma unroll 4
        for (int i = j + lane; i < mr; i += 64) cc[i] -= d * vs[i];
      }
    }
    __syncthreads();
  }

  // ---- G[l][j] = v_l . v_j (l < j): v_j is 1 at row j and 0 above it
  float* G = qsm;
  for (int p = wave; p < jb * jb; p += QR_THREADS / 64) {
    const int l = p / jb, j = p - l * jb;
    if (l >= j) continue;
    const float* cl = P + (int64_t)l * m;
    const float* cj = P + (int64_t)j * m;
    float d = 0.f;
#pragma unroll 4
    for (int i = j + 1 + lane; i < mr; i += 64) d += cl[i] * cj[i];
    d = wave_sum(d);
    if (lane == 0) G[l * NB + j] = d + cl[j];
  }
  __syncthreads();
  // ---- T[i][i] = tau_i, T[:j, j] = -tau_j T[:j, :j] G[:j, j]: thread i owns row i (it depends on no other row)
  if (tid < NB) {
    const int i = tid;
    float trow[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      float t = 0.f;
      if (j < jb && j >= i) {   // j < jb is uniform
        if (j == i) {
          t = taus[j];
        } else {
          float s = 0.f;
#pragma unroll
          for (int l = 0; l < j; ++l) s += trow[l] * G[l * NB + j];   // trow[l] = 0 for l < i
          const float tj = taus[j];
          t = tj != 0.f ? -tj * s : 0.f;
        }
      }
      trow[j] = t;
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) T[i * NB + j] = i < jb ? trow[j] : 0.f;
  }
}

// C[:, c] <- (I - V op(T) V^T) C[:, c] for ncols columns; op(T) = T^T (trans) or T.  V[j * m + i], C[c * m + i], rows i < mr.
__global__ __launch_bounds__(QRB_THREADS) void qr_larfb_kernel(const float* __restrict__ V, const float* __restrict__ T,
                                                               float* __restrict__ C, int m, int mr, int jb, int ncols,
                                                               int trans) {
  constexpr int NB = QRB_NB, NC = QRB_NC, JPW = NB / QRB_WAVES;
  __shared__ __attribute__((aligned(16))) float Tsh[NB * NB];
  __shared__ __attribute__((aligned(16))) float Wsh[NB * NC];
  __shared__ __attribute__((aligned(16))) float W2sh[NB * NC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c0 = blockIdx.x * NC;
  const int nc = ncols - c0 < NC ? ncols - c0 : NC;
  float* Cc[NC];   // columns past the last one alias it: loaded, never stored
#pragma unroll
  for (int c = 0; c < NC; ++c) Cc[c] = C + (int64_t)(c0 + (c < nc ? c : nc - 1)) * m;
  for (int e = tid; e < NB * NB; e += QRB_THREADS) Tsh[e] = T[e];

  // ---- phase 1: W = V^T C
  {
    float acc[JPW][NC];
    const float* Vj[JPW];
    int jcol[JPW];
#pragma unroll
    for (int jj = 0; jj < JPW; ++jj) {
      jcol[jj] = wave + QRB_WAVES * jj;
      Vj[jj] = V + (int64_t)(jcol[jj] < jb ? jcol[jj] : jb - 1) * m;
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[jj][c] = 0.f;
    }
    for (int i = lane; i < mr; i += 64) {
      float cv[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) cv[c] = Cc[c][i];
#pragma unroll
      for (int jj = 0; jj < JPW; ++jj) {
        const int j = jcol[jj];
        float v = Vj[jj][i];
        v = i > j ? v : (i == j ? 1.f : 0.f);
        v = j < jb ? v : 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[jj][c] = fmaf(v, cv[c], acc[jj][c]);
      }
    }
#pragma unroll
    for (int jj = 0; jj < JPW; ++jj)
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const float s = wave_sum(acc[jj][c]);
        if (lane == 0) Wsh[jcol[jj] * NC + c] = s;
      }
  }
  __syncthreads();

  // ---- phase 2: W2 = op(T) W (T upper triangular: only its triangle is summed)
  if (tid < NB * NC) {
    const int j = tid / NC, c = tid - j * NC;
    float s = 0.f;
    if (j < jb) {
      if (trans) {
        for (int l = 0; l <= j; ++l) s = fmaf(Tsh[l * NB + j], Wsh[l * NC + c], s);
      } else {
        for (int l = j; l < jb; ++l) s = fmaf(Tsh[j * NB + l], Wsh[l * NC + c], s);
      }
    }
    W2sh[tid] = s;
  }
  __syncthreads();

  // ---- phase 3: C -= V W2
  for (int i = tid; i < mr; i += QRB_THREADS) {
    float s[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) s[c] = 0.f;
    const float* vrow = V + i;
    if (i >= jb) {
#pragma unroll 4
      for (int j = 0; j < jb; ++j) {
        const float v = vrow[(int64_t)j * m];
        const f32x4 w0 = *(const f32x4*)&W2sh[j * NC], w1 = *(const f32x4*)&W2sh[j * NC + 4];
        s[0] = fmaf(v, w0[0], s[0]), s[1] = fmaf(v, w0[1], s[1]), s[2] = fmaf(v, w0[2], s[2]), s[3] = fmaf(v, w0[3], s[3]);
        s[4] = fmaf(v, w1[0], s[4]), s[5] = fmaf(v, w1[1], s[5]), s[6] = fmaf(v, w1[2], s[6]), s[7] = fmaf(v, w1[3], s[7]);
      }
    } else {
      for (int j = 0; j <= i; ++j) {   // v[i][j] = 0 for j > i
        const float v = j == i ? 1.f : vrow[(int64_t)j * m];
#pragma unroll
        for (int c = 0; c < NC; ++c) s[c] = fmaf(v, W2sh[j * NC + c], s[c]);
      }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < nc) Cc[c][i] -= s[c];
  }
}
static_assert(QRB_NC == 8, "phase 3 of qr_larfb_kernel is written out for 8 columns");

// Qt[c * m + i] = (i == c)
__global__ void qr_eye_kernel(float* Qt, int m, int r) {
  const int64_t n = (int64_t)m * r;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx / m), i = (int)(idx - (int64_t)c * m);
    Qt[idx] = i == c ? 1.f : 0.f;
  }
}

static int grid_for(int64_t n) {
  int64_t g = (n + 255) / 256;
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  return (int)g;
}

static size_t qr_block_panel_lds(int m) {
  const size_t fl = (size_t)m > (size_t)QRB_NB * QRB_NB ? (size_t)m : (size_t)QRB_NB * QRB_NB;
  return fl * sizeof(float);
}

// Factor W[:, :kc] and form Q[:, :r] as launch_qr_panel does.  Pt: [kc * m] floats, Qt: [r * m] floats, T: qr_blocked_t_floats(kc).
int launch_qr_blocked(const void* W, int64_t ldw, int in_dtype, int m, int kc, int r, float* Pt, float* Qt, float* T,
                      hipStream_t stream) {
  if (m <= 0 || kc <= 0 || r <= 0 || kc > m || r > m) return SOW_ERR_SHAPE;
  if (qr_block_panel_lds(m) > 150 * 1024) return SOW_ERR_UNSUPPORTED;   // m > 38400: the limit of the one-workgroup panel too
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
  SOW_SET_MAX_LDS_ONCE(150 * 1024, qr_block_panel_kernel);
  const int nblk = ceil_div(kc, QRB_NB);
  for (int b = 0; b < nblk; ++b) {
    const int j0 = b * QRB_NB, jb = kc - j0 < QRB_NB ? kc - j0 : QRB_NB;
    float* Tb = T + (size_t)b * QRB_NB * QRB_NB;
    hipLaunchKernelGGL(qr_block_panel_kernel, dim3(1), dim3(QR_THREADS), qr_block_panel_lds(m - j0), stream, Pt, Tb, m, j0, jb);
    SOW_CHECK_LAUNCH();
    const int ntrail = kc - j0 - jb;
    if (ntrail > 0) {
      hipLaunchKernelGGL(qr_larfb_kernel, dim3(ceil_div(ntrail, QRB_NC)), dim3(QRB_THREADS), 0, stream,
                         Pt + (int64_t)j0 * m + j0, Tb, Pt + (int64_t)(j0 + jb) * m + j0, m, m - j0, jb, ntrail, 1);
      SOW_CHECK_LAUNCH();
    }
  }
  hipLaunchKernelGGL(qr_eye_kernel, dim3(grid_for((int64_t)m * r)), dim3(256), 0, stream, Qt, m, r);
  SOW_CHECK_LAUNCH();
  for (int b = nblk - 1; b >= 0; --b) {
    // columns of Qt left of j0 are still unit vectors with zeros in rows >= j0: H_b leaves them alone
    const int j0 = b * QRB_NB, jb = kc - j0 < QRB_NB ? kc - j0 : QRB_NB;
    hipLaunchKernelGGL(qr_larfb_kernel, dim3(ceil_div(r - j0, QRB_NC)), dim3(QRB_THREADS), 0, stream,
                       Pt + (int64_t)j0 * m + j0, T + (size_t)b * QRB_NB * QRB_NB, Qt + (int64_t)j0 * m + j0, m, m - j0, jb,
                       r - j0, 0);
    SOW_CHECK_LAUNCH();
  }
  return SOW_OK;
}

}  // namespace sow
