// Dense product for ragged leading dimensions (bf16 / f16):  C[M, N] = A[M, K] . op(B),  alpha = 1, beta = 0, no bias.
//
// The dense-accumulator term of a layer whose d_in or d_out is not a multiple of 8 (llama_1b's 5461-wide MLP):
//   NN  B stored [K][N]:  y  = x  . W_acc      (2048 -> 5461: N, ldb, ldc ragged; 5461 -> 2048: K, lda ragged)
//   NT  B stored [N][K]:  dX = dY . W_acc^T    (2048 -> 5461: K, lda, ldb ragged; 5461 -> 2048: N, ldc ragged)
// lda / ldb / ldc are any element counts, so a row starts at any 2-byte offset; the bases are 16-byte aligned.  W_acc is
// read in place: no copy, no workspace.
//
// 128 x 128 tile, 256 threads (2 x 2 waves, 64 x 64 per wave = 2 x 2 v_mfma_f32_32x32x16), BK = 64, two workgroups per CU,
// XCD-aware tile order with N fastest (gemm.hip).  Both operands are staged global -> registers -> LDS with ONE register
// set: tile t + 1 is written after the barrier that ends the products of tile t - 1, tile t + 2 is issued at once and
// stays in flight under the products of tile t + 1.
//
// Loads: whole aligned 16-byte pieces through a buffer descriptor that spans only what the workgroup may read -- its 128
// rows of a k-contiguous operand, or all K rows of its 128 columns of the k-major B (rag_load.hpp).  The piece that
// crosses the end of the tensor is read dword by dword and nothing past the end is requested.
//   k-contiguous (A; B of the NT form): a thread holds 32 consecutive k of one row = 5 pieces, shifted into place in
//     registers and written as four 16-byte chunks of the LDS image;
//   k-major (B of the NN form): a thread holds 16 consecutive n of two consecutive k rows = 2 x 3 pieces, realigned along n,
//     then transposed in registers (the 8x2 transpose of the generic k-major loader): 16 dwords (n, k pair) of the image.
// Elements at k >= K are zeroed in BOTH operands: the bytes after a row's end are the next row's data and 0 x NaN is NaN.
// Rows m >= M / columns n >= N hold whatever the descriptor returns; they only reach accumulators that are never stored.
//
// LDS image (both operands): Img[row][64 k], 128-byte rows of eight 16-byte chunks, physical chunk =
// c ^ (row >> 1 & 7) ^ (row >> 4 & 7).  The first term is the swizzle of bf16_img_off<64> (ds_read_b128 fragment reads of 16
// consecutive rows touch 16 different slots); the second spreads the dword writes of the transposed loader, whose lanes
// write rows 16 apart, over all chunks (2-way conflicts instead of 8-way).
//
// Stores: C is written once, RNE from the fp32 accumulator.  A ragged C row (ldc or N not a multiple of 8) shares its
// boundary dwords with its neighbours, so it is written element by element with 2-byte stores: no byte of another tile is
// written or read.  Aligned C takes the 16-byte row-segment stores of the generic epilogue.
#include "kernels.hpp"
#include "epilogue.hpp"
#include "rag_load.hpp"
#include <type_traits>

namespace sow {

struct RagGemmParams {
  const void *A, *B;
  void* C;
  int64_t M, lda, ldb, ldc;
  int N, K;
  int nt_store;
};

constexpr int RG_BM = 128, RG_BN = 128, RG_BK = 64, RG_IMG = 128 * RG_BK * 2;

__device__ __forceinline__ int rg_off(int row, int c) { return row * 128 + ((c ^ (row >> 1) ^ (row >> 4)) & 7) * 16; }

// [128 rows x 64 k] tile of a k-contiguous operand: thread t holds k = 32 (t & 1) .. + 31 of row t >> 1
struct RagTileKC {
  RagSpan<5> s;
  int n;   // elements of the span below K

  __device__ __forceinline__ void load(__amdgpu_buffer_rsrc_t rs, uint32_t lim, int rows, int64_t ld, int k0, int K, int t) {
    const int row = t >> 1, gk = k0 + (t & 1) * 32;
    n = K - gk;
    if (row < rows && n > 0) s.load(rs, lim, (uint32_t)row * (uint32_t)ld + (uint32_t)gk);
    else s.zero(), n = 0;
  }
  __device__ __forceinline__ void store(char* img, int t) const {
    uint32_t d[16];
    s.get(d, n);
    const int row = t >> 1, c0 = (t & 1) * 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) *(u32x4*)(img + rg_off(row, c0 + q)) = u32x4{d[4 * q], d[4 * q + 1], d[4 * q + 2], d[4 * q + 3]};
  }
};

// [64 k x 128 n] tile of the k-major operand: thread t holds n = 16 (t & 7) .. + 15 of the k rows 2 (t >> 3), + 1
struct RagTileKM {
  RagSpan<3> s[2];

  __device__ __forceinline__ void load(__amdgpu_buffer_rsrc_t rs, uint32_t lim, int64_t ld, int k0, int K, int t) {
    const int k = k0 + 2 * (t >> 3), nc = (t & 7) * 16;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (k + i < K) s[i].load(rs, lim, (uint32_t)(k + i) * (uint32_t)ld + (uint32_t)nc);
      else s[i].zero();
    }
  }
  __device__ __forceinline__ void store(char* img, int t) const {
    uint32_t r0[8], r1[8];
    s[0].get(r0, 16);
    s[1].get(r1, 16);
    const int kp = t >> 3, nc = (t & 7) * 16;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const uint32_t lo = (r0[q] & 0xffffu) | (r1[q] << 16), hi = (r0[q] >> 16) | (r1[q] & 0xffff0000u);
      *(uint32_t*)(img + rg_off(nc + 2 * q, kp >> 2) + (kp & 3) * 4) = lo;
      *(uint32_t*)(img + rg_off(nc + 2 * q + 1, kp >> 2) + (kp & 3) * 4) = hi;
    }
  }
};

// NT: B stored [N][K];  VECC: ldc and N multiples of 8 (16-byte stores)
template <typename T, bool NT, bool VECC> __global__ __launch_bounds__(256, 2) void gemm_rag_kernel(const RagGemmParams p) {
  using V8 = typename DT<T>::v8;
  constexpr int SCR = EpiScratch<2>::FLOATS * 4;
  constexpr int LDS = 2 * RG_IMG > 4 * SCR ? 2 * RG_IMG : 4 * SCR;
  __shared__ __attribute__((aligned(16))) char smem[LDS];
  char* As = smem;
  char* Bs = smem + RG_IMG;

  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int wm = w >> 1, wn = w & 1, li = lane & 31, lh = lane >> 5;
  const int tiles_n = (p.N + RG_BN - 1) / RG_BN;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t m0 = (int64_t)(lid / tiles_n) * RG_BM;
  const int n0 = (lid % tiles_n) * RG_BN;
  const T* A = (const T*)p.A;
  const T* B = (const T*)p.B;

  // descriptors over what this workgroup may read (bases 16-byte aligned: m0 and n0 are multiples of 128)
  const int rows_a = p.M - m0 < RG_BM ? (int)(p.M - m0) : RG_BM;
  const uint32_t lim_a = (uint32_t)(((int64_t)(rows_a - 1) * p.lda + p.K) * 2);
  const __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc((void*)(A + m0 * p.lda), (short)0, (int)lim_a, 0x00020000);
  const int rows_b = p.N - n0 < RG_BN ? p.N - n0 : RG_BN;
  // NT: rows n0 .. of [N][K]; NN: columns n0 .. of every k row, up to the end of the tensor
  const uint32_t lim_b = NT ? (uint32_t)(((int64_t)(rows_b - 1) * p.ldb + p.K) * 2)
                            : (uint32_t)(((int64_t)(p.K - 1) * p.ldb + (p.N - n0)) * 2);
  const __amdgpu_buffer_rsrc_t rs_b =
      __builtin_amdgcn_make_buffer_rsrc((void*)(NT ? B + (int64_t)n0 * p.ldb : B + n0), (short)0, (int)lim_b, 0x00020000);

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

  RagTileKC ta;
  typename std::conditional<NT, RagTileKC, RagTileKM>::type tb;
  auto load = [&](int k0) {
    ta.load(rs_a, lim_a, rows_a, p.lda, k0, p.K, t);
    if constexpr (NT) tb.load(rs_b, lim_b, rows_b, p.ldb, k0, p.K, t);
    else tb.load(rs_b, lim_b, p.ldb, k0, p.K, t);
  };
  const int nk = (p.K + RG_BK - 1) / RG_BK;
  load(0);
  for (int kt = 0; kt < nk; ++kt) {
    ta.store(As, t);
    tb.store(Bs, t);
    __syncthreads();
    if (kt + 1 < nk) load((kt + 1) * RG_BK);
#pragma unroll
    for (int ks = 0; ks < RG_BK / 16; ++ks) {
      const V8 a0 = *(const V8*)(As + rg_off(wm * 64 + li, 2 * ks + lh));
      const V8 a1 = *(const V8*)(As + rg_off(wm * 64 + 32 + li, 2 * ks + lh));
      const V8 b0 = *(const V8*)(Bs + rg_off(wn * 64 + li, 2 * ks + lh));
      const V8 b1 = *(const V8*)(Bs + rg_off(wn * 64 + 32 + li, 2 * ks + lh));
      acc[0][0] = mfma32(a0, b0, acc[0][0]);
      acc[0][1] = mfma32(a0, b1, acc[0][1]);
      acc[1][0] = mfma32(a1, b0, acc[1][0]);
      acc[1][1] = mfma32(a1, b1, acc[1][1]);
    }
    __syncthreads();
  }
  float* scratch = (float*)(smem + w * SCR);
#pragma unroll
  for (int mh = 0; mh < 2; ++mh)
    wave_store_tiles<T, 2, VECC>(acc[mh], scratch, (T*)p.C, p.ldc, m0 + wm * 64 + mh * 32, n0 + wn * 64, p.M, p.N, 1.f, 0.f,
                                 (const T*)nullptr, lane, p.nt_store != 0);
}

// bf16 / f16, 16-byte aligned bases, leading dimensions that cover the rows; every descriptor offset stays below 2^31:
// 128 rows of a k-contiguous operand, K rows of the k-major one
bool gemm_rag_supported(const void* A, int64_t lda, const void* B, int64_t ldb, bool transB, const void* C, int64_t ldc, int64_t M,
                        int N, int K, int dtype) {
  if (dtype != SOW_BF16 && dtype != SOW_F16) return false;
  if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0) return false;
  if (!al16p(A) || !al16p(B) || !al16p(C)) return false;
  if (lda < K || ldb < (transB ? K : N) || ldc < N) return false;
  constexpr int64_t LIM = (int64_t)1 << 31;
  if (RG_BM * lda * 2 >= LIM) return false;
  if ((transB ? RG_BN * ldb : (int64_t)K * ldb) * 2 >= LIM) return false;
  return (int64_t)ceil_div(M, RG_BM) * ceil_div(N, RG_BN) <= 0x7fffffff;
}

template <typename T> static void launch_rag_t(const RagGemmParams& p, bool transB, bool vecc, unsigned tiles, hipStream_t stream) {
  const dim3 grid(tiles), block(256);
  if (transB) {
    if (vecc) hipLaunchKernelGGL((gemm_rag_kernel<T, true, true>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((gemm_rag_kernel<T, true, false>), grid, block, 0, stream, p);
  } else {
    if (vecc) hipLaunchKernelGGL((gemm_rag_kernel<T, false, true>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((gemm_rag_kernel<T, false, false>), grid, block, 0, stream, p);
  }
}

int launch_gemm_rag(const void* A, int64_t lda, const void* B, int64_t ldb, bool transB, void* C, int64_t ldc, int64_t M, int N,
                    int K, int dtype, hipStream_t stream) {
  if (!gemm_rag_supported(A, lda, B, ldb, transB, C, ldc, M, N, K, dtype)) return SOW_ERR_UNSUPPORTED;
  RagGemmParams p;
  p.A = A, p.B = B, p.C = C, p.M = M, p.lda = lda, p.ldb = ldb, p.ldc = ldc, p.N = N, p.K = K;
  p.nt_store = SOW_GEMM_NT(M) ? 1 : 0;
  const bool vecc = ldc % 8 == 0 && N % 8 == 0;
  const unsigned tiles = (unsigned)((int64_t)ceil_div(M, RG_BM) * ceil_div(N, RG_BN));
  if (dtype == SOW_BF16) launch_rag_t<bf16_t>(p, transB, vecc, tiles, stream);
  else launch_rag_t<f16_t>(p, transB, vecc, tiles, stream);
  SOW_CHECK_LAUNCH();
  return SOW_OK;
}

}  // namespace sow
