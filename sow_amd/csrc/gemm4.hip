// bf16 GEMM with an optional K-extension, two wave groups in anti-phase (gfx950):
//     C[M,N] = alpha * (A[M,K] . op(B) + A2[M,64] . op(B2)) + beta * C + bias[N]
// Same contract as gemm2.hip (the dense-accumulator form of the SoW layer, tn_gradient/layer/sow.py:109-121 as ONE
// fp32-accumulated product: y = [x, h] . [W_acc; B], dX = [dY, dh] . [W_acc^T; A^T]); a different main loop.
//
// Why another main loop.  gemm2 / gemm3 advance K in 32-wide stages with one barrier per stage and run at 36-50 % of the
// matrix pipe: every wave loads, waits and multiplies in the same rhythm, so the pipe idles while the fragments and the
// DMA issue go out.  Here (the structure of the CDNA guide's 256 x 256 "8-phase" template, rebuilt for this contract):
//   * 256 x 256 tile, K in 64-wide tiles, 8 waves = 2 (rows) x 4 (columns), 128 x 64 per wave, v_mfma_f32_16x16x32_bf16 (the
//     f16 entry symbols: v_mfma_f32_16x16x32_f16, the same body otherwise)
//     (the chip holds a higher clock on it than on 32x32x16 at equal cycles per flop);
//   * the two wave ROWS run one barrier apart: between two barriers one group issues its 16 MFMAs of a 64 x 32 quadrant
//     while the other (its SIMD partners) reads the next quadrant's fragments and issues the DMA of one half-tile;
//   * a K-tile lives in LDS as four 16-KiB half-tiles cut along the quadrant boundaries -- A0 / A1 = the first / second 64
//     rows of BOTH wave rows, B0 / B1 = the first / second 32 columns of ALL FOUR wave columns -- so that a half-tile is
//     read in exactly one phase of its K-tile and its slot can be re-filled two phases later: quadrant order (0,0) (0,1)
//     (1,1) (1,0) reads A0 + B0, B1, A1, nothing; phase P issues the DMA of half-tile P + 6 (order A0 B0 B1 A1 per tile),
//     2 x 64 KiB ring = 8 slots, up to 5 half-tiles (80 KiB) in flight per CU;
//   * counted waits only: after its DMA issue every phase waits for vmcnt(8) = everything but the four youngest
//     half-tiles, which is exactly what phase P + 1 reads; that wait is followed by two barriers before the read (the
//     groups are one barrier apart);
//   * k-contiguous half-tiles are [128][64] images (128-byte rows), 16-byte chunk c of row r at c ^ ((r >> 1) & 7):
//     every ds_read_b128 lane group touches 16 distinct 16-byte slots; the k-major B of the forward product stays k-major
//     ([64 k][128 n], 256-byte rows, chunk c of k-row k at c ^ (((k & 3) | ((k >> 3) & 1) << 2) << 1)) and is read
//     with ds_read_b64_tr_b16.  The XOR sits on the per-lane SOURCE address (LDS-DMA writes lane-linearly);
//   * the products are computed TRANSPOSED (the W fragment is the MFMA's A operand): a lane then holds 4 consecutive
//     output columns of one token row, the epilogue parks 16 x 64 blocks in a wave-private LDS scratch with four
//     16-byte writes and stores whole 128-byte row segments;
//   * per-lane source pointers for the eight DMA instructions of a K-tile are carried in registers and advanced by one
//     64-bit add; rows / columns beyond the matrix are CLAMPED (they only feed outputs that are never stored); the K tail
//     and the extension tile take a checked path that reads the zero page where k is out of range;
//   * short M (config 5: T = 1024 -> 64 tiles for a 4096-wide output) runs split-K: S blocks per tile, each on a K range,
//     fp32 partial products through the caller's workspace, summed in split order by a second, chip-wide launch.
#include "kernels.hpp"
#include "lds_dma.hpp"
#include <type_traits>

namespace sow {

constexpr int G4_BM = 256, G4_BN = 256, G4_BK = 64;
constexpr int G4_THREADS = 512;
constexpr int G4_HALF = 128 * G4_BK * 2;   // 16 KiB
constexpr int G4_BUF = 4 * G4_HALF;        // 64 KiB: A0 | A1 | B0 | B1
constexpr int G4_LDS = 2 * G4_BUF;         // 128 KiB
constexpr int G4_OFF_A0 = 0, G4_OFF_A1 = G4_HALF, G4_OFF_B0 = 2 * G4_HALF, G4_OFF_B1 = 3 * G4_HALF;
constexpr int G4_SCR_LD = 68;              // floats per scratch row (64 + 4: 16-byte aligned rows, staggered banks)
constexpr int G4_SCR = 16 * G4_SCR_LD * 4; // bytes of one wave's epilogue scratch
constexpr int G4_HIMG = G4_LDS;            // gemm4h: the projected [256][64] tile, two half images of 16 KiB behind the ring
constexpr int G4_LDS_H = G4_LDS + 2 * G4_HALF;   // 160 KiB
constexpr int G4_PA_BUF = 2 * G4_HALF + 8192;    // gemm4h projection pass: A0 | A1 | F (8 KiB) per K-tile, three buffers in the ring

// The operand and output pointers are 16-bit storage: bf16 for gemm4_kernel, f16 bit patterns for gemm4_f16_kernel (the kernel
// body moves them as raw 16-bit words and converts only where it does arithmetic -- the MFMA, the epilogue, the H rounding).
struct Gemm4Params {
  const bf16_t* A;
  const bf16_t* B;
  const bf16_t* A2;   // [M, 64] or nullptr
  const bf16_t* B2;   // NT: [N, 64]; NN: [k2, N]
  bf16_t* C;
  const bf16_t* bias;
  int64_t M, lda, ldb, lda2, ldb2, ldc;
  int N, K, k2;
  int k2e;            // NT: valid k columns of B2's rows (64: zero-padded rows; r: raw [N][r] rows, gemm4h)
  float alpha, beta;
  int nt_store;
  // HF = true (gemm4h): the rank-r projection H = hscale * A . op(F) is computed by the kernel itself and is the extension's
  // A operand (A2 is not read): F is [r, K] (NT, ld ldf) or a zero-padded [K, 64] (NN, ld ldf); Hout [M, 64] receives the
  // saved copy (column 63 <- 1.0 when r < 64) from the first column tile
  const bf16_t* F;
  int64_t ldf;
  bf16_t* Hout;
  int r;
  float hscale;
  // split-K (short M: fewer output tiles than CUs).  splits > 1: block b = split * tiles + tile runs K-tiles
  // [split * kt_per, ...) of its tile and leaves the fp32 sum of that range in partials[split][M][N]; a second launch
  // (gemm4_splitk_reduce_kernel, every CU) adds the splits in order and applies alpha / beta / bias.
  int splits, kt_per;
  float* partials;
};

__device__ __forceinline__ f32x4 mfma16(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(a), as_bf16x8(b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma16_f16(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(as_v8<f16_t>(a), as_v8<f16_t>(b), c, 0, 0, 0);
}

// LDS reads with compile-time immediate offsets (inline asm: invisible to hipcc's vmcnt bookkeeping, see lds_dma.hpp)
template <int OFF> __device__ __forceinline__ void g4_rd128(u32x4& d, uint32_t a) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(a), "n"(OFF) : "memory");
}
template <int OFF> __device__ __forceinline__ void g4_rdtr(u32x2& d, uint32_t a) {
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(d) : "v"(a), "n"(OFF) : "memory");
}
// x fragments of row half MH: 4 row tiles x 2 k-steps
template <int MH> __device__ __forceinline__ void g4_read_a(u32x4 (&af)[4][2], uint32_t a0, uint32_t a1) {
  g4_rd128<MH * G4_HALF + 0 * 2048>(af[0][0], a0);
  g4_rd128<MH * G4_HALF + 0 * 2048>(af[0][1], a1);
  g4_rd128<MH * G4_HALF + 1 * 2048>(af[1][0], a0);
  g4_rd128<MH * G4_HALF + 1 * 2048>(af[1][1], a1);
  g4_rd128<MH * G4_HALF + 2 * 2048>(af[2][0], a0);
  g4_rd128<MH * G4_HALF + 2 * 2048>(af[2][1], a1);
  g4_rd128<MH * G4_HALF + 3 * 2048>(af[3][0], a0);
  g4_rd128<MH * G4_HALF + 3 * 2048>(af[3][1], a1);
}
// W fragments of column half NH from a k-contiguous image: 2 column tiles x 2 k-steps
template <int NH> __device__ __forceinline__ void g4_read_b_nt(u32x4 (&bf)[2][2], uint32_t b0, uint32_t b1) {
  g4_rd128<NH * G4_HALF + 0 * 2048>(bf[0][0], b0);
  g4_rd128<NH * G4_HALF + 0 * 2048>(bf[0][1], b1);
  g4_rd128<NH * G4_HALF + 1 * 2048>(bf[1][0], b0);
  g4_rd128<NH * G4_HALF + 1 * 2048>(bf[1][1], b1);
}
// ... from a k-major image (transposed reads): [nt][ks] low / high k quads
template <int NH> __device__ __forceinline__ void g4_read_b_nn(u32x2 (&bl)[2][2], u32x2 (&bh)[2][2], uint32_t n0a, uint32_t n1a) {
  g4_rdtr<NH * G4_HALF + 0>(bl[0][0], n0a);
  g4_rdtr<NH * G4_HALF + 1024>(bh[0][0], n0a);
  g4_rdtr<NH * G4_HALF + 8192>(bl[0][1], n0a);
  g4_rdtr<NH * G4_HALF + 8192 + 1024>(bh[0][1], n0a);
  g4_rdtr<NH * G4_HALF + 0>(bl[1][0], n1a);
  g4_rdtr<NH * G4_HALF + 1024>(bh[1][0], n1a);
  g4_rdtr<NH * G4_HALF + 8192>(bl[1][1], n1a);
  g4_rdtr<NH * G4_HALF + 8192 + 1024>(bh[1][1], n1a);
}

// kinds of half-tile, in DMA issue order within a K-tile
enum : int { G4_A0 = 0, G4_B0 = 1, G4_B1 = 2, G4_A1 = 3 };
template <int KIND> __device__ __forceinline__ constexpr int g4_slot_off() {
  return KIND == G4_A0 ? G4_OFF_A0 : KIND == G4_A1 ? G4_OFF_A1 : KIND == G4_B0 ? G4_OFF_B0 : G4_OFF_B1;
}

#define G4_KERNEL gemm4_kernel
#define G4_REDUCE gemm4_splitk_reduce_kernel
#define G4_T bf16_t
#define G4_MFMA mfma16
#define G4_PACK pack_bf16x2
#define G4_ONE 0x3F80u
#include "gemm4_body.hpp"
#undef G4_KERNEL
#undef G4_REDUCE
#undef G4_T
#undef G4_MFMA
#undef G4_PACK
#undef G4_ONE
// the f16 forms: v_mfma_f32_16x16x32_f16 and RNE rounding to f16, the same code otherwise
#define G4_KERNEL gemm4_f16_kernel
#define G4_REDUCE gemm4_f16_splitk_reduce_kernel
#define G4_T f16_t
#define G4_MFMA mfma16_f16
#define G4_PACK pack_f16x2
#define G4_ONE 0x3C00u
#include "gemm4_body.hpp"
#undef G4_KERNEL
#undef G4_REDUCE
#undef G4_T
#undef G4_MFMA
#undef G4_PACK
#undef G4_ONE

// ------------------------------------------------------------------------------------------------
bool gemm4_supported(const ExtGemm& g, int dtype) {
  if (dtype != SOW_BF16 && dtype != SOW_F16) return false;
  return g.M >= 1 && g.N >= 64 && g.K >= 64 && ext_gemm_operands_ok(g);
}

// split-K plan for an M x N x K product with an optional K-extension tile: splits (1 = none) and K-tiles per split.  Taken
// when the output has at most 128 tiles (half of the CUs idle otherwise) and K >= 6144: the partial products cost a write and
// a read of S x M x N fp32 whatever K is -- ~33 us at 1024 x 4096, S = 4 -- so at K = 4096 the split (56-58 us) only ties with
// gemm3s's 256 small tiles (53-55 us) and is not worth its 64 MB of scratch; at K = 11008 it runs 90-93 us against 121-125
// (profiles/r03_gemm_splitk.txt).  Up to four splits, at least 8 K-tiles each.
static int gemm4_split_plan(int64_t M, int N, int K, bool has_ext, int* kt_per) {
  const int64_t tiles = (int64_t)ceil_div(M, G4_BM) * ceil_div(N, G4_BN);
  const int ntl = ceil_div(K, G4_BK) + (has_ext ? 1 : 0);
  *kt_per = ntl;
  if (tiles <= 0 || tiles > 128 || ntl < 96 || sw_on(SW_NO_SPLITK)) return 1;
  int s = (int)(256 / tiles);
  if (s > 4) s = 4;
  while (s > 1 && ntl / s < 8) --s;
  if (s <= 1) return 1;
  *kt_per = ceil_div(ntl, s);
  return ceil_div(ntl, *kt_per);
}
size_t gemm4_splitk_bytes(int64_t M, int N, int K, bool has_ext) {
  int kt_per;
  const int s = gemm4_split_plan(M, N, K, has_ext, &kt_per);
  if (s <= 1) return 0;
  return (size_t)s * (size_t)M * (size_t)N * sizeof(float) + 256;
}
int gemm4_splits(int64_t M, int N, int K, bool has_ext, const void* ws, size_t ws_bytes) {
  int kt_per;
  const int s = gemm4_split_plan(M, N, K, has_ext, &kt_per);
  return (s > 1 && ws && ws_bytes >= gemm4_splitk_bytes(M, N, K, has_ext)) ? s : 1;
}

int launch_gemm4(const ExtGemm& g, int dtype, void* ws, size_t ws_bytes, hipStream_t stream) {
  if (dtype != SOW_BF16 && dtype != SOW_F16) return SOW_ERR_DTYPE;
  const bool f16 = dtype == SOW_F16, nt = g.nt;
  const int64_t M = g.M;
  const int N = g.N, K = g.K;
  Gemm4Params p;
  p.A = (const bf16_t*)g.A, p.B = (const bf16_t*)g.B, p.A2 = (const bf16_t*)g.A2, p.B2 = (const bf16_t*)g.B2;
  p.C = (bf16_t*)g.C, p.bias = (const bf16_t*)g.bias;
  p.M = M, p.lda = g.lda, p.ldb = g.ldb, p.lda2 = g.lda2, p.ldb2 = g.ldb2, p.ldc = g.ldc;
  p.N = N, p.K = K, p.k2 = g.k2 < 64 ? g.k2 : 64;
  p.k2e = 64;
  p.alpha = g.alpha, p.beta = g.beta;
  p.nt_store = SOW_GEMM_NT(M) ? 1 : 0;
  p.F = nullptr, p.ldf = 0, p.Hout = nullptr, p.r = 0, p.hscale = 0.f;
  p.splits = 1, p.kt_per = 0, p.partials = nullptr;
  const int64_t tiles = (int64_t)ceil_div(M, G4_BM) * ceil_div(N, G4_BN);
  if (tiles <= 0) return SOW_OK;
  if (tiles > 0x7fffffff) return SOW_ERR_SHAPE;
  int64_t grid = tiles;
  if (gemm4_splits(M, N, K, g.A2 != nullptr, ws, ws_bytes) > 1) {
    p.splits = gemm4_split_plan(M, N, K, g.A2 != nullptr, &p.kt_per);
    p.partials = (float*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    grid = tiles * p.splits;
  }
#define G4_LAUNCH(K, LDS, ...)                                                                                   \
  do {                                                                                                           \
    SOW_SET_MAX_LDS_ONCE(LDS, K<__VA_ARGS__>);                                                                   \
    hipLaunchKernelGGL((K<__VA_ARGS__>), dim3((unsigned)grid), dim3(G4_THREADS), LDS, stream, p);               \
  } while (0)
  if (p.splits > 1 && nt) {
    if (f16) G4_LAUNCH(gemm4_f16_kernel, G4_LDS, true, false, true);
    else G4_LAUNCH(gemm4_kernel, G4_LDS, true, false, true);
  } else if (p.splits > 1) {
    if (f16) G4_LAUNCH(gemm4_f16_kernel, G4_LDS, false, false, true);
    else G4_LAUNCH(gemm4_kernel, G4_LDS, false, false, true);
  } else if (nt) {
    if (f16) G4_LAUNCH(gemm4_f16_kernel, G4_LDS, true, false);
    else G4_LAUNCH(gemm4_kernel, G4_LDS, true, false);
  } else {
    if (f16) G4_LAUNCH(gemm4_f16_kernel, G4_LDS, false, false);
    else G4_LAUNCH(gemm4_kernel, G4_LDS, false, false);
  }
  SOW_CHECK_LAUNCH();
  if (p.splits > 1) {
    const int64_t work = M * (N / 8);
    const dim3 rgrid((unsigned)((work + 255) / 256));
    if (f16)
      hipLaunchKernelGGL(gemm4_f16_splitk_reduce_kernel, rgrid, dim3(256), 0, stream, p.partials, p.splits, M, N, (f16_t*)p.C, p.ldc,
                         (const f16_t*)p.bias, p.alpha, p.beta);
    else
      hipLaunchKernelGGL(gemm4_splitk_reduce_kernel, rgrid, dim3(256), 0, stream, p.partials, p.splits, M, N, p.C, p.ldc, p.bias,
                         p.alpha, p.beta);
    SOW_CHECK_LAUNCH();
  }
  return SOW_OK;
}

// ---- gemm4h: C = X . op(W) + H . op(G) + bias with H = hscale * X . op(F) computed in the kernel and saved -------------
// NN (forward: y = x W_acc + h B): W [K, N], F = A zero-padded to [K, 64] (ldf = 64), G = B [r, N].
// NT (backward: dX = dY W_acc^T + dh A^T): W [N, K], F = B [r, K], G = A zero-padded to [N, 64] (ldg = 64).
bool gemm4h_supported(const ProjGemm& g, bool nt, int dtype) {
  if ((dtype != SOW_BF16 && dtype != SOW_F16) || !g.X || !g.W || !g.F || !g.G || !g.C || !g.H) return false;
  if (sw_on(SW_NO_FUSED_H) || sw_on(SW_FORCE_GEMM_V1) || sw(SW_GEMM4) == 0 || sw_on(SW_NO_GEMM4H)) return false;
  if (g.r < 2 || g.r > 64 || (g.r & 1) || g.N < 64 || g.K < 64) return false;   // r even: A's 2r-byte rows stay 4-byte aligned
  const int tiles_n = ceil_div(g.N, G4_BN);
  // every column tile repeats the projection pass (the row panel streams in once more per tile): one or two tiles
  if (tiles_n > 2 || (int64_t)ceil_div(g.M, G4_BM) * tiles_n < 120) return false;
  if (g.K % 8 || g.N % 8 || g.ldx % 8 || g.ldw % 8 || g.ldc % 8) return false;
  if (!al16p(g.X) || !al16p(g.W) || !al16p(g.C) || !al16p(g.H) || !al16p(g.bias)) return false;
  if (nt) {   // F = B [r, K] (16-byte pieces along rows), G = A [N, r] as stored (or zero-padded to 64 columns)
    if (g.ldf % 8 || !al16p(g.F) || !al4p(g.G) || (g.ldg != g.r && g.ldg != 64)) return false;
  } else {    // F = A [K, r] as stored (or [K, 64]), G = B [r, N]
    if (g.ldg % 8 || !al16p(g.G) || !al4p(g.F) || (g.ldf != g.r && g.ldf != 64)) return false;
  }
  return true;
}

int launch_gemm4h(const ProjGemm& g, bool nt, int dtype, hipStream_t stream) {
  if (dtype != SOW_BF16 && dtype != SOW_F16) return SOW_ERR_DTYPE;
  const bool f16 = dtype == SOW_F16;
  Gemm4Params p;
  p.A = (const bf16_t*)g.X, p.B = (const bf16_t*)g.W, p.A2 = nullptr, p.B2 = (const bf16_t*)g.G;
  p.C = (bf16_t*)g.C, p.bias = (const bf16_t*)g.bias;
  p.M = g.M, p.lda = g.ldx, p.ldb = g.ldw, p.lda2 = 64, p.ldb2 = g.ldg, p.ldc = g.ldc;
  p.N = g.N, p.K = g.K, p.k2 = g.r < 64 ? g.r : 64;
  p.k2e = nt ? (g.ldg == 64 ? 64 : g.r) : 64;
  p.alpha = 1.f, p.beta = 0.f;
  p.nt_store = SOW_GEMM_NT(g.M) ? 1 : 0;
  p.F = (const bf16_t*)g.F, p.ldf = g.ldf, p.Hout = (bf16_t*)g.H, p.r = g.r, p.hscale = g.hscale;
  p.splits = 1, p.kt_per = 0, p.partials = nullptr;
  const int64_t tiles = (int64_t)ceil_div(g.M, G4_BM) * ceil_div(g.N, G4_BN);
  if (tiles <= 0) return SOW_OK;
  if (tiles > 0x7fffffff) return SOW_ERR_SHAPE;
  const int64_t grid = tiles;
  if (nt) {
    if (f16) G4_LAUNCH(gemm4_f16_kernel, G4_LDS_H, true, true);
    else G4_LAUNCH(gemm4_kernel, G4_LDS_H, true, true);
  } else {
    if (f16) G4_LAUNCH(gemm4_f16_kernel, G4_LDS_H, false, true);
    else G4_LAUNCH(gemm4_kernel, G4_LDS_H, false, true);
  }
#undef G4_LAUNCH
  SOW_CHECK_LAUNCH();
  return SOW_OK;
}

}  // namespace sow
