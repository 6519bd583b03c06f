// Fused forward for generation-sized inputs (T <= 32 tokens): bf16 / f16, r_live <= 64, dense accumulator or none.
//
//   h = rn( scale * sum_k x[t,k] A[k,j] )                               fp32 sum, rounded once to the compute dtype
//   y = rn( sum_k x[t,k] W[k,n] + sum_j h[t,j] B[j,n] + bias[n] )       fp32 sum, rounded ONCE
//
// At these token counts the call is a stream of W (2 d_in d_out bytes) with next to no arithmetic per byte, so the grid is
// cut over the WEIGHT, not over tokens:
//
//   phase A (skinny_a_kernel)  one workgroup per (64-column range of d_out) x (K-slab of d_in); the slab length is planned
//       on the host so that the layer has >= 512 workgroups where its size allows (skinny_plan).  The workgroup stages its
//       slab of x in LDS ([16 or 32 rows][KS], rows >= T and k >= d_in are zeros made here, never memory read past x);
//       its four waves take the slab's 32-deep k-steps in turn.  A wave reads 32 rows x 64 columns of W per step straight
//       into registers -- every lane 8 bytes of one row, 16 lanes = 128 contiguous bytes of a W row, non-temporal, each
//       byte of W read exactly once by the whole grid -- and turns the 8 rows a lane holds into the four B fragments of
//       v_mfma_f32_16x16x32_bf16 / _f16 with byte permutes (lane l: k = 8 (l >> 4) + i down the register, column
//       4 (l & 15) + c for fragment c; the permutation of columns inside the range is undone when the tile is parked).  x
//       is the A operand (one or two 16-row tiles).  The four waves' fp32 tiles are added in wave order through LDS and
//       the sum goes to the workspace as the slab's partial product Py[s][t][n].
//       A wave requests its first four k-steps before the x slab is staged, so the whole slab of a 4096 x 4096 layer is in
//       flight from the first instruction on.
//       The first S * ceil(r / 16) workgroups of a layer compute the partial sums of one 16-column tile of x . A instead
//       (Ph[s][t][64]): A is [d_in][r] with any r, so its fragments are gathered with 2-byte loads; same x staging, same
//       MFMA, same reduction.
//   phase B (skinny_b_kernel)  one workgroup per 64 columns x 4 token rows, one output element per thread: h = rn(scale *
//       sum_s Ph[s]) of its four rows into LDS, then per output element the slab partials in slab order, the r products
//       h . B in order of j, the bias, one rounding, one store.
//
// No atomics, fixed summation order: a repeat gives the same bits, and a layer inside a group (grid concatenation, per-layer
// block offset) computes exactly what it computes alone.
//
// E4M3 accumulator (SOW_ACC_DENSE_FP8, the SK_FP8 / FP8 = true instantiations): W is the codes, one byte per element, and the column
// exponents come with it.  Phase A reads a lane's 8 bytes of a row -- 8 columns, 16 lanes = 128 contiguous bytes, so a column
// range is 128 wide and a wave holds eight 16-column tiles -- converts the codes UNSCALED to the compute dtype in registers
// (v_cvt_pk_f32_fp8, then the upper halves / v_cvt_pkrtz: every E4M3 value is a bf16 and an f16 number, no rounding happens)
// and feeds the same MFMA; Py holds sum x . q.  Phase B multiplies the slab-order sum of column n by 2^e_n (exact in fp32)
// before h . B and the bias.  Everything else -- x staging, the x . A workgroups, the reduction, the order of every sum -- is
// the code above.
//
// MXFP4 accumulator (SOW_ACC_DENSE_FP4, the SK_FP4 instantiations of phase A): W is packed E2M1 codes, one byte = rows k, k + 1
// of one column, and one E8M0 scale byte per (32-row block, column) comes with it.  The geometry is the E4M3 one -- 8-byte
// loads of 8 columns, 128-column ranges -- but a lane's 8 bytes are a row PAIR: four loads per 32-deep step (one MX block)
// instead of eight, plus one 8-byte load of the block's scale bytes.  v_cvt_scalef32_pk_{bf16,f16}_fp4 turns one byte and the
// scale into a fragment register (two rows of one column): 32 conversions per step, no packs.  The scale is applied in the
// conversion, so Py holds sum x . W^ and phase B is the plain one.
//
// fp32 factors (SOW_PARAM_F32 | SOW_ACC_NATIVE, the PF = true instantiations of both kernels, for every accumulator format): A, B
// and the bias are fp32 master copies and the accumulator is what it is above.  No pack launch: the x . A workgroups gather A
// with 4-byte loads into the register the 2-byte load fills (the raw bits wait there while x is staged) and round at first use;
// phase B loads its column of B and the bias as fp32 and rounds where the fmaf reads them.  One rounding per value, to nearest
// even (from_f32<T>, the rounding of the parameter pack): y is bit-identical to the PF = false call on pre-rounded factors.
//
// 33 <= T <= 64 (sow_forward_skinny_rows, the RT = 4 instantiations of phase A, for every format and factor dtype): a wave holds
// three or four 16-row tiles of x (the x slab is 48 or 64 rows) and feeds every fragment of W, built or converted ONCE, to four
// MFMAs (the fourth tile of a 48-row slab is zeros in a register: no branch around its MFMA).  The four waves' tiles are parked
// and added in two passes of 32 rows -- 4 x 32 x 132 floats = 66 KiB for a 128-column range -- in the same wave order.  The slab
// plan is skinny_rows_plan (below): slabs of at most 768 rows at T <= 48 and 512 above keep the x slab under half a CU's LDS.
// A plain accumulator keeps two workgroups per CU (230 registers); four row tiles of codes hold 128 accumulator registers next
// to the operand ring and run one workgroup per CU (SOW_SKINNY_ROWS_OCC8).  Phase B is the kernel above on a
// larger grid.  Layers of at most 32 rows in such a call are launched as a group of their own through the RT = 2 forms.
//
// Short batches WITH gradients (sow_forward_short / sow_backward_short, SOW_ACC_DENSE, 1 <= T <= 1024): a layer is
// cut into row blocks of 64, every block one SkLayer entry on the same W with a slab plan counted over the blocks
// (short_rows_plan).  The forward is the RT = 4 plain phase A as it is and the SK_SH_FWD form of phase B, which also stores the
// h rows it has rounded (h_save).  The data gradient is the TR = true form of phase A (skinny_a_tr: dY staged as x, W_acc read
// transposed in place) and the SK_SH_BWD form of phase B (skinny_b_tr: dh to memory, dX = rn(sum Py + dh . A^T)).
//
// The same on codes read in place (sow_forward_short_codes / sow_backward_short_codes, SOW_ACC_DENSE_FP8 / _FP4): the
// forward is the RT = 4 code form of phase A per row block (128-column ranges, short_codes_plan) and SK_SH_FWD of phase B, with the
// E4M3 column scaling where the format asks for it.  The data gradient keeps the plain geometry and dequantises W in registers to the
// exact bits of the image (skinny_a_tr_codes: the scale varies along the contraction there), so phase B is the plain SK_SH_BWD and dX,
// dh are bit-identical to sow_backward_short on the image.
#include <type_traits>

#include "kernels.hpp"

namespace sow {

#ifndef SOW_SKINNY_NCT
#define SOW_SKINNY_NCT 4   // 16-column MFMA tiles per wave: 4 (8-byte loads, 64-column ranges) or 8 (16-byte loads, 128)
#endif
constexpr int SK_NCT = SOW_SKINNY_NCT;
constexpr int SK_NCT8 = 8;                // ... of an E4M3 accumulator: 8-byte loads of 8 columns, 128-column ranges
constexpr int SK_KSTEP = 32;              // k per MFMA step
constexpr int SK_KQ = 4 * SK_KSTEP;       // k per round of the four waves
constexpr int SK_KS_MAX = 1024;           // longest K-slab (x slab in LDS: 32 x 1032 x 2 bytes)
constexpr int SK_XPAD = 8;                // elements of padding per staged x row
constexpr int SK_WANT_WGS = 512;          // two workgroups per CU
#ifndef SOW_SKINNY_WANT8
#define SOW_SKINNY_WANT8 512
#endif
constexpr int SK_WANT_WGS8 = SOW_SKINNY_WANT8;   // ... of an E4M3 accumulator (256 and 1024 each win some shapes and lose others: DESIGN 4.5b)
constexpr int SK_BN = 64;                 // columns per phase-B workgroup
// how the dense accumulator of a call is stored: in the compute dtype, as E4M3 codes, or as packed E2M1 codes (MXFP4)
enum SkFmt : int { SK_PLAIN = 0, SK_FP8 = 1, SK_FP4 = 2 };
// what a lane holds of one row of W (one row pair of MXFP4 codes): NCT columns in NDW dwords
template <SkFmt F> struct SkW {
  static constexpr int NCT = SK_NCT8, NDW = 2;
  typedef __attribute__((ext_vector_type(2))) uint32_t vec;
};
template <> struct SkW<SK_PLAIN> {
  static constexpr int NCT = SK_NCT, NDW = SK_NCT / 2;
  typedef __attribute__((ext_vector_type(SK_NCT / 2))) uint32_t vec;
};
constexpr int sk_cn(bool codes) { return 16 * (codes ? SK_NCT8 : SK_NCT); }   // columns per phase-A workgroup
constexpr int sk_rs(bool codes) { return sk_cn(codes) + 4; }   // row pitch (floats) of the parked tiles: 4 rows apart = 16 banks apart
constexpr SkFmt sk_fmt(int acc_kind) { return acc_kind == SOW_ACC_DENSE_FP8 ? SK_FP8 : acc_kind == SOW_ACC_DENSE_FP4 ? SK_FP4 : SK_PLAIN; }

struct SkGroup {
  SkLayer L[SK_MAXL];
  int n;
};
static_assert(sizeof(SkGroup) <= 4096, "by-value kernel arguments must stay under 4 KiB");

void skinny_plan(int d_in, int d_out, int acc_kind, int* S, int* KS, int* ncr) {
  const bool codes = acc_is_codes(acc_kind);
  const int nc = acc_kind == SOW_ACC_DENSE || codes ? ceil_div(d_out, sk_cn(codes)) : 0;
  const int want = nc ? ceil_div(codes ? SK_WANT_WGS8 : SK_WANT_WGS, nc) : 32;
  int ks = ceil_div(ceil_div(d_in, want), SK_KQ) * SK_KQ;
  if (ks < SK_KQ) ks = SK_KQ;
  if (ks > SK_KS_MAX) ks = SK_KS_MAX;
  *KS = ks, *S = ceil_div(d_in, ks), *ncr = nc;
}

template <typename T> __device__ __forceinline__ f32x4 sk_mfma(u32x4 a, u32x4 b, f32x4 c);
template <> __device__ __forceinline__ f32x4 sk_mfma<bf16_t>(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_v8<bf16_t>(a), as_v8<bf16_t>(b), c, 0, 0, 0);
}
template <> __device__ __forceinline__ f32x4 sk_mfma<f16_t>(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(as_v8<f16_t>(a), as_v8<f16_t>(b), c, 0, 0, 0);
}

template <typename V> __device__ __forceinline__ V sk_load_w(const V* p) {
#ifdef SOW_SKINNY_NO_NT
  return *p;
#else
  return __builtin_nontemporal_load(p);
#endif
}

// two fp32 values that ARE numbers of T (converted E4M3 codes) as a pair of T: nothing is rounded
template <typename T> __device__ __forceinline__ uint32_t sk_pack_exact(float lo, float hi);
template <> __device__ __forceinline__ uint32_t sk_pack_exact<bf16_t>(float lo, float hi) {
  return __builtin_amdgcn_perm(__float_as_uint(hi), __float_as_uint(lo), 0x07060302u);
}
template <> __device__ __forceinline__ uint32_t sk_pack_exact<f16_t>(float lo, float hi) {
  const auto h = __builtin_amdgcn_cvt_pkrtz(lo, hi);
  uint32_t u;
  __builtin_memcpy(&u, &h, 4);
  return u;
}

// fp32 factors (PF = true instantiations, SOW_PARAM_F32 | SOW_ACC_NATIVE): one fp32 element, rounded once to nearest even to T,
// as the 16 bits the kernels would have loaded from a packed copy (the rounding of the parameter pack, misc.hip)
template <typename T> __device__ __forceinline__ uint32_t sk_rn_bits(float v) {
  const T t = from_f32<T>(v);
  uint16_t u;
  __builtin_memcpy(&u, &t, 2);
  return u;
}

// a parameter element as phase B uses it: of T as loaded, or fp32 rounded once to T
template <typename T, typename TP> __device__ __forceinline__ float sk_param(TP v) {
  if constexpr (std::is_same<TP, T>::value) return to_f32(v);
  else return to_f32(from_f32<T>(v));
}

constexpr int SK_PF = 4;   // k-steps a wave keeps in flight: all of them are requested before the x slab is staged
// Four row tiles of codes hold 128 accumulator registers, and the compiler needs about 390 for the whole wave: one wave per
// SIMD (one workgroup per CU), with the same four k-steps in flight.  Two per SIMD (256 registers) spill, at any depth of the
// ring: -DSOW_SKINNY_ROWS_OCC8=2 -DSOW_SKINNY_ROWS_PF8=2 builds that form for the A/B of DESIGN 4.5d.
#ifndef SOW_SKINNY_ROWS_PF8
#define SOW_SKINNY_ROWS_PF8 SK_PF
#endif
#ifndef SOW_SKINNY_ROWS_OCC8
#define SOW_SKINNY_ROWS_OCC8 1
#endif

// The second argument of __launch_bounds__: the least number of waves per SIMD the compiler has to leave room for.  With two
// row tiles it is 1, which asks for nothing -- one wave per SIMD is what __launch_bounds__(256) alone guarantees, and the
// RT = 2 forms keep the registers and occupancy they had without it.  With four row tiles: two for a plain
// accumulator, SOW_SKINNY_ROWS_OCC8 for codes.  (A table, because the attribute takes no template-id with a comma.)
// by [SkFmt][RT / 4]
constexpr int SK_OCC[3][2] = {{1, 2}, {1, SOW_SKINNY_ROWS_OCC8}, {1, SOW_SKINNY_ROWS_OCC8}};
// ---- short batches, data gradient (sow_backward_short): the TR = true instantiations of phase A (plain format, RT = 4) ----
//   dh = rn(scale . dY B^T),  dX = rn(dY W_acc^T + dh A^T)
// The roles are swapped on the host (launch_skinny_short): L.x = dY [T][K], K = the layer's d_out = the contraction, L.d_out = N =
// the layer's d_in; a K-slab is a range of the layer's d_out, a column range 64 columns of its d_in.  W_acc is read in place: the B
// operand of v_mfma_f32_16x16x32 wants eight consecutive contraction elements of one output column per lane, and for W_acc^T
// those are W_acc[n0 + (l & 15)][k0 + 8 (l >> 4) .. + 7] -- one aligned 16-byte load, no byte permutes.  A wave takes its k-steps
// in PAIRS (SK_TR_KC = 64 deep per wave and round): the two loads of a tile ask for the 128 contiguous bytes of a W row together,
// non-temporal, every byte of W read once per row block.  The first S * ceil(r / 16) workgroups compute dY . B^T instead: the
// fragment of column j is B[j][k .. k + 7], again one 16-byte load (B is [r][d_out]: no 2-byte gather).  x staging, MFMA, the
// park and the wave-order reduction are those of the forward; an accumulator tile's column IS the local column here.
constexpr int SK_TR_KC = 2 * SK_KSTEP;   // k per wave and round
constexpr int SK_TR_KQ = 4 * SK_TR_KC;   // k per round of the four waves (SK_SHORT_KQ_BWD)
constexpr int SK_TR_PF = 2;              // rounds a wave keeps in flight: all of a slab of at most 512
static_assert(SK_TR_KQ == SK_SHORT_KQ_BWD, "the data gradient's slabs are whole rounds");
// PONLY: the dY . B^T workgroups alone, as the code forms call them (one tile: the W tiles' registers are not held)
template <typename T, bool PONLY = false> __device__ __forceinline__ void skinny_a_tr(const SkGroup& g, char* sk_smem) {
  constexpr int RT = 4, NCT = PONLY ? 1 : 4, CN = 64, RS = sk_rs(false);
  int li = 0;
  for (int i = 1; i < g.n; ++i)
    if ((int)blockIdx.x >= g.L[i].startA) li = i;
  const SkLayer& L = g.L[li];
  const int b = (int)blockIdx.x - L.startA;
  const int ntj = (L.r + 15) >> 4;            // 16-column tiles of dY . B^T
  const bool is_p = PONLY || b < L.S * ntj;   // the first S * ntj workgroups: (slab, tile) of dY . B^T
  const int s = is_p ? b / ntj : (b - L.S * ntj) / L.ncr;
  const int cr = is_p ? b % ntj : (b - L.S * ntj) % L.ncr;
  const int Tn = L.T, K = L.d_in, N = L.d_out, KS = L.KS, r = L.r;
  const int rows = Tn > 48 ? 64 : 48;
  const bool live3 = rows == 64;              // the fourth row tile holds rows of the call
  const int kbeg = s * KS;
  const int klen = min(KS, K - kbeg);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n16 = lane & 15, kg = lane >> 4;
  const int kk0 = w * SK_TR_KC;

  // ---- requests first ----
  // tile c of W: row n = 64 cr + 16 c + n16 of W_acc (clamped: a row past N is not requested); dY . B^T: row j = 16 cr + n16 of B
  const T* rowp[NCT];
  bool ok[NCT];
#pragma unroll
  for (int c = 0; c < NCT; ++c) {
    const int n = is_p ? cr * 16 + n16 : cr * CN + c * 16 + n16;
    const int lim = is_p ? r : N;
    ok[c] = n < lim && (c == 0 || !is_p);
    rowp[c] = (const T*)(is_p ? L.A : L.W) + (size_t)min(n, lim - 1) * K;
  }
  u32x4 d[SK_TR_PF][NCT][2];
  auto load_round = [&](int kk, u32x4(&o)[NCT][2]) {
#pragma unroll
    for (int c = 0; c < NCT; ++c)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int kq = kk + q * SK_KSTEP, k = kbeg + kq + kg * 8;   // K is a multiple of 8: a lane's eight are all in or all out
        u32x4 v = {0u, 0u, 0u, 0u};
        if (ok[c] && kq < klen && k < K) {
          if (is_p) v = *(const u32x4*)(rowp[c] + k);               // B is read by every slab's workgroups of every block: cached
          else v = sk_load_w((const u32x4*)(rowp[c] + k));
        }
        o[c][q] = v;
      }
  };
#pragma unroll
  for (int p = 0; p < SK_TR_PF; ++p) load_round(kk0 + p * SK_TR_KQ, d[p]);

  // ---- the slab of dY: [rows][KS + pad], zeros for t >= T and k >= K ----
  const int xpitch = (KS + SK_XPAD) * 2;   // bytes
  {
    const T* x = (const T*)L.x;
    const int cpr = KS / 8;
    for (int idx = tid; idx < rows * cpr; idx += 256) {
      const int t = idx / cpr, c = idx - t * cpr, k = kbeg + c * 8;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (t < Tn && k < K) v = *(const u32x4*)(x + (size_t)t * K + k);
      *(u32x4*)(sk_smem + t * xpitch + c * 16) = v;
    }
  }
  __syncthreads();

  f32x4 acc[NCT][RT];
#pragma unroll
  for (int c = 0; c < NCT; ++c)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc[c][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const char* xa0 = sk_smem + n16 * xpitch + kg * 16;
  for (int kb = kk0; kb < klen; kb += SK_TR_PF * SK_TR_KQ) {
#pragma unroll
    for (int p = 0; p < SK_TR_PF; ++p) {
      const int kk = kb + p * SK_TR_KQ;
      if (kk < klen) {   // uniform per wave
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int kq = kk + q * SK_KSTEP;   // (< KS: slabs are whole rounds; past klen both operands are zeros)
          u32x4 a[RT];
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) {
            a[rt] = u32x4{0u, 0u, 0u, 0u};
            if (rt < 3 || live3) a[rt] = *(const u32x4*)(xa0 + rt * 16 * xpitch + kq * 2);
          }
#pragma unroll
          for (int c = 0; c < NCT; ++c)
            if (c == 0 || !is_p) {
#pragma unroll
              for (int rt = 0; rt < RT; ++rt) acc[c][rt] = sk_mfma<T>(a[rt], d[p][c][q], acc[c][rt]);
            }
        }
        load_round(kk + SK_TR_PF * SK_TR_KQ, d[p]);   // (requests nothing past the slab)
      }
    }
  }

  // ---- park the four waves' tiles in two passes of 32 rows, add them in wave order, store the slab partial ----
  __syncthreads();
  float* red = (float*)sk_smem;
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
    if (ps) __syncthreads();
#pragma unroll
    for (int c = 0; c < NCT; ++c)
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
        if ((2 * ps + hf < 3 || live3) && (c == 0 || !is_p)) {
#pragma unroll
          for (int q = 0; q < 4; ++q) red[(w * 32 + hf * 16 + kg * 4 + q) * RS + c * 16 + n16] = acc[c][2 * ps + hf][q];
        }
    __syncthreads();
    const int t0 = 32 * ps, tn = min(Tn - t0, 32);
    if (!is_p) {
      float* Py = L.Py + ((size_t)s * Tn + t0) * N;
      for (int idx = tid; idx < tn * CN; idx += 256) {
        const int t = idx / CN, jc = idx - t * CN;
        const int n = cr * CN + jc;
        float v = red[t * RS + jc];
#pragma unroll
        for (int ww = 1; ww < 4; ++ww) v += red[(ww * 32 + t) * RS + jc];
        if (n < N) Py[(size_t)t * N + n] = v;
      }
    } else {
      float* Ph = L.Ph + ((size_t)s * Tn + t0) * 64 + cr * 16;
      for (int idx = tid; idx < tn * 16; idx += 256) {
        const int t = idx >> 4, jj = idx & 15;
        float v = red[t * RS + jj];
#pragma unroll
        for (int ww = 1; ww < 4; ++ww) v += red[(ww * 32 + t) * RS + jj];
        Ph[t * 64 + jj] = v;
      }
    }
  }
}

// ---- the same on codes (sow_backward_short_codes): the W workgroups of the TR = true instantiations with F = SK_FP8 / SK_FP4 ----
// The geometry above is kept -- contraction = the layer's d_out, 64-column ranges of its d_in, the k-to-wave partition with each wave's k
// pair, the park, the wave-order reduction -- and a fragment is dequantised in registers to the exact bits of the image W^ (the scale
// varies along the contraction here: it cannot wait for phase B).  The sums therefore see the operands sow_backward_short sees on
// the image, in the same order: dX and dh are bit-identical to it.  The dY . B^T workgroups are the plain ones (skinny_a_tr<T, true>).
//   E4M3   a lane's fragment = codes[n][k .. k + 7], one 8-byte non-temporal load per tile; the eight exponents exps[k .. k + 7], one
//          8-byte load per k-step for the four tiles (cached: every workgroup of the slab reads them).  v_cvt_pk_f32_fp8, v_ldexp_f32
//          (never a multiply: fused into a conversion it loses the sign of -0) and the pack of the forward, which rounds nothing.
//   MXFP4  a byte of codes[n / 2][k] = rows n and n + 1 of column k: one 8-byte load gives eight contraction elements of TWO output
//          columns, their scale bytes are scales[n / 32][k .. k + 7].  The scaled conversion of byte k with ITS scale yields (row n,
//          row n + 1) of that k; four v_perm_b32 per parity gather the low halves (row n) and the high halves (row n + 1) into two
//          fragments.  A wave's four tiles are the even and odd rows of two groups of 16 code rows (32 rows of d_in each, one MX
//          block): tile 2 g + parity, tile column n16 = local column 32 g + 2 n16 + parity, undone where the sum is stored.
// A row past N is not requested (N is a multiple of 32 for MXFP4: a group is whole or absent).
#ifndef SOW_SHORT_CODES_NQ
#define SOW_SHORT_CODES_NQ 2
#endif
template <typename T, SkFmt F> __device__ __forceinline__ void skinny_a_tr_codes(const SkGroup& g, char* sk_smem) {
  static_assert(F == SK_FP8 || F == SK_FP4, "a code format");
  constexpr bool FP4 = F == SK_FP4;
  constexpr int RT = 4, NCT = 4, CN = 64, RS = sk_rs(false);
  constexpr int NLD = FP4 ? 2 : 4;   // code loads per k-step: groups of 16 code rows, or tiles
  constexpr int NSC = FP4 ? 2 : 1;   // scale loads per k-step: one per group (its MX block), or the step's column exponents
  // k-steps a wave takes per round: 2 = the plain form's pairs (64-byte pieces of a code row, its summation partition: the bit
  // identity); 4 = the A/B of DESIGN 4.5f (128-byte pieces, one round in flight, another partition of the sum)
  constexpr int NQ = SOW_SHORT_CODES_NQ, KC = NQ * SK_KSTEP, KQ = 4 * KC, PF = NQ == 2 ? SK_TR_PF : 1;
  static_assert(NQ == 2 || NQ == 4, "pairs or fours");
  typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
  int li = 0;
  for (int i = 1; i < g.n; ++i)
    if ((int)blockIdx.x >= g.L[i].startA) li = i;
  const SkLayer& L = g.L[li];
  const int b = (int)blockIdx.x - L.startA - L.S * ((L.r + 15) >> 4);   // (>= 0: the caller took the dY . B^T workgroups)
  const int s = b / L.ncr, cr = b % L.ncr;
  const int Tn = L.T, K = L.d_in, N = L.d_out, KS = L.KS;
  const int rows = Tn > 48 ? 64 : 48;
  const bool live3 = rows == 64;
  const int kbeg = s * KS;
  const int klen = min(KS, K - kbeg);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n16 = lane & 15, kg = lane >> 4;
  const int kk0 = w * KC;

  // ---- requests first ----
  const char* cp[NLD];   // the lane's row of codes (K bytes per row, per row pair of MXFP4)
  const char* sp[NSC];
  bool ok[NLD];
#pragma unroll
  for (int u = 0; u < NLD; ++u) {
    if constexpr (FP4) {
      const int n0 = cr * CN + u * 32;   // the group's first row of d_in
      ok[u] = n0 < N;
      const int nc0 = min(n0, N - 32);
      cp[u] = (const char*)L.W + (size_t)((nc0 >> 1) + n16) * K;
      sp[u] = (const char*)L.wexp + (size_t)(nc0 >> 5) * K;
    } else {
      const int n = cr * CN + u * 16 + n16;
      ok[u] = n < N;
      cp[u] = (const char*)L.W + (size_t)min(n, N - 1) * K;
    }
  }
  if constexpr (!FP4) sp[0] = (const char*)L.wexp;
  u32x2 d[PF][NQ][NLD + NSC];
  auto load_round = [&](int kk, u32x2(&o)[NQ][NLD + NSC]) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int kq = kk + q * SK_KSTEP, k = kbeg + kq + kg * 8;   // K is a multiple of 8: a lane's eight are all in or all out
      const bool in = kq < klen && k < K;
#pragma unroll
      for (int u = 0; u < NLD; ++u) {
        u32x2 v = {0u, 0u};
        if (ok[u] && in) v = sk_load_w((const u32x2*)(cp[u] + k));
        o[q][u] = v;
      }
#pragma unroll
      for (int u = 0; u < NSC; ++u) {
        u32x2 v = {0u, 0u};
        if (in) v = *(const u32x2*)(sp[u] + k);
        o[q][NLD + u] = v;
      }
    }
  };
#pragma unroll
  for (int p = 0; p < PF; ++p) load_round(kk0 + p * KQ, d[p]);

  // ---- the slab of dY: [rows][KS + pad], zeros for t >= T and k >= K ----
  const int xpitch = (KS + SK_XPAD) * 2;   // bytes
  {
    const T* x = (const T*)L.x;
    const int cpr = KS / 8;
    for (int idx = tid; idx < rows * cpr; idx += 256) {
      const int t = idx / cpr, c = idx - t * cpr, k = kbeg + c * 8;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (t < Tn && k < K) v = *(const u32x4*)(x + (size_t)t * K + k);
      *(u32x4*)(sk_smem + t * xpitch + c * 16) = v;
    }
  }
  __syncthreads();

  f32x4 acc[NCT][RT];
#pragma unroll
  for (int c = 0; c < NCT; ++c)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc[c][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const char* xa0 = sk_smem + n16 * xpitch + kg * 16;
  for (int kb = kk0; kb < klen; kb += PF * KQ) {
#pragma unroll
    for (int p = 0; p < PF; ++p) {
      const int kk = kb + p * KQ;
      if (kk < klen) {   // uniform per wave
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const int kq = kk + q * SK_KSTEP;
          u32x4 a[RT];
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) {
            a[rt] = u32x4{0u, 0u, 0u, 0u};
            if (rt < 3 || live3) a[rt] = *(const u32x4*)(xa0 + rt * 16 * xpitch + kq * 2);
          }
          auto mma = [&](int c, const u32x4& f) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) acc[c][rt] = sk_mfma<T>(a[rt], f, acc[c][rt]);
          };
          if constexpr (FP4) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
              const u32x2 qv = d[p][q][u], sv = d[p][q][NLD + u];
              uint32_t pr[8];   // k element j: row n in the low half, row n + 1 in the high half
#pragma unroll
              for (int j = 0; j < 8; ++j) {
                const float sc = __uint_as_float(((sv[j >> 2] >> (8 * (j & 3))) & 0xffu) << 23);   // E8M0 byte -> 2^e
                pr[j] = cvt_fp4_pair<T>(qv[j >> 2], sc, j & 3);
              }
              u32x4 fe, fo;
#pragma unroll
              for (int m = 0; m < 4; ++m) {
                fe[m] = __builtin_amdgcn_perm(pr[2 * m + 1], pr[2 * m], 0x05040100u);
                fo[m] = __builtin_amdgcn_perm(pr[2 * m + 1], pr[2 * m], 0x07060302u);
              }
              mma(2 * u, fe);
              mma(2 * u + 1, fo);
            }
          } else {
            const u32x2 ev = d[p][q][NLD];
            int e[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) e[j] = (int)(int8_t)(ev[j >> 2] >> (8 * (j & 3)));
#pragma unroll
            for (int c = 0; c < NCT; ++c) {
              const u32x2 qv = d[p][q][c];
              u32x4 f;
#pragma unroll
              for (int wd = 0; wd < 2; ++wd) {
                const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8(qv[wd], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(qv[wd], true);
                f[2 * wd] = sk_pack_exact<T>(__builtin_ldexpf(lo[0], e[4 * wd]), __builtin_ldexpf(lo[1], e[4 * wd + 1]));
                f[2 * wd + 1] = sk_pack_exact<T>(__builtin_ldexpf(hi[0], e[4 * wd + 2]), __builtin_ldexpf(hi[1], e[4 * wd + 3]));
              }
              mma(c, f);
            }
          }
        }
        load_round(kk + PF * KQ, d[p]);   // (requests nothing past the slab)
      }
    }
  }

  // ---- park the four waves' tiles in two passes of 32 rows, add them in wave order, store the slab partial ----
  __syncthreads();
  float* red = (float*)sk_smem;
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
    if (ps) __syncthreads();
#pragma unroll
    for (int c = 0; c < NCT; ++c)
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
        if (2 * ps + hf < 3 || live3) {
#pragma unroll
          for (int q = 0; q < 4; ++q) red[(w * 32 + hf * 16 + kg * 4 + q) * RS + c * 16 + n16] = acc[c][2 * ps + hf][q];
        }
    __syncthreads();
    const int t0 = 32 * ps, tn = min(Tn - t0, 32);
    float* Py = L.Py + ((size_t)s * Tn + t0) * N;
    for (int idx = tid; idx < tn * CN; idx += 256) {
      const int t = idx / CN, jc = idx - t * CN;
      const int n = cr * CN + jc;
      // MXFP4: local column jc = 32 g + 2 n16 + parity sits in tile 2 g + parity, tile column n16
      const int slot = FP4 ? (((jc >> 5) * 2 + (jc & 1)) * 16 + ((jc & 31) >> 1)) : jc;
      float v = red[t * RS + slot];
#pragma unroll
      for (int ww = 1; ww < 4; ++ww) v += red[(ww * 32 + t) * RS + slot];
      if (n < N) Py[(size_t)t * N + n] = v;
    }
  }
}

// RT = the 16-row tiles of x a wave holds: 2 (T <= 32, one or two live) or 4 (33 <= T <= 64, three or four live)
// TR: the data gradient of short batches (skinny_a_tr / skinny_a_tr_codes above; RT = 4 only, every format: two waves per SIMD as the plain form)
template <typename T, SkFmt F = SK_PLAIN, bool PF = false, int RT = 2, bool TR = false> __global__ __launch_bounds__(256, SK_OCC[TR ? SK_PLAIN : F][RT / 4]) void skinny_a_kernel(const SkGroup g) {
  extern __shared__ __align__(16) char sk_smem[];
  static_assert(!TR || (!PF && RT == 4), "the transposed form exists with four row tiles and factors of T");
  if constexpr (TR) {   // (what follows is dead code in these instantiations)
    if constexpr (F == SK_PLAIN) {
      skinny_a_tr<T>(g, sk_smem);
    } else {
      int li = 0;
      for (int i = 1; i < g.n; ++i)
        if ((int)blockIdx.x >= g.L[i].startA) li = i;
      const SkLayer& L = g.L[li];
      if ((int)blockIdx.x - L.startA < L.S * ((L.r + 15) >> 4)) skinny_a_tr<T, true>(g, sk_smem);   // dY . B^T: the plain workgroups
      else skinny_a_tr_codes<T, F>(g, sk_smem);
    }
    return;
  }
  constexpr bool FP8 = F == SK_FP8, FP4 = F == SK_FP4;
  constexpr int SK_NCT = SkW<F>::NCT, SK_CN = sk_cn(F != SK_PLAIN), SK_RS = sk_rs(F != SK_PLAIN);
  typedef typename SkW<F>::vec sk_wvec;
  int li = 0;
  for (int i = 1; i < g.n; ++i)
    if ((int)blockIdx.x >= g.L[i].startA) li = i;
  const SkLayer& L = g.L[li];
  const int b = (int)blockIdx.x - L.startA;
  const int ntj = (L.r + 15) >> 4;            // 16-column tiles of x . A
  const bool is_xa = b < L.S * ntj;           // the first S * ntj workgroups: (slab, tile) of x . A
  // column range fastest: workgroups that start together read neighbouring 128-byte pieces of the same rows of W
  const int s = is_xa ? b / ntj : (b - L.S * ntj) / L.ncr;
  const int cr = is_xa ? b % ntj : (b - L.S * ntj) % L.ncr;   // tile of x . A, or column range of W
  const int Tn = L.T, d_in = L.d_in, d_out = L.d_out, KS = L.KS;
  const int rows = RT == 2 ? (Tn > 16 ? 32 : 16) : (Tn > 48 ? 64 : 48);
  // row tile rt holds rows of the call (uniform per layer); tile 0, and with RT = 4 tiles 1 and 2, always do
  auto live = [&](int rt) { return RT == 2 ? rows == 32 : (rt < 3 || rows == 64); };
  const int kbeg = s * KS;
  const int klen = min(KS, d_in - kbeg);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n16 = lane & 15, kg = lane >> 4;
  const int kk0 = w * SK_KSTEP;

  // ---- requests first: the operand stream does not depend on x ----
  // W: lane = rows k0 + 8 kg + i, columns col0 .. col0 + NCT - 1.  x . A: lane = the same rows, column j of A, one element.
  constexpr int NPF = (RT == 4 && F != SK_PLAIN) ? SOW_SKINNY_ROWS_PF8 : SK_PF;
  sk_wvec d[NPF][8];
  const int col0 = cr * SK_CN + n16 * SK_NCT;
  const bool col_ok = col0 < d_out;   // d_out is a multiple of 8, NCT of 4 (8 for E4M3): a lane's columns are all in or all out
  const char* Wp = (const char*)L.W + (size_t)col0 * (F != SK_PLAIN ? 1 : sizeof(T));
  const size_t wpitch = (size_t)d_out * (F != SK_PLAIN ? 1 : sizeof(T));   // bytes per row of W (per row pair of MXFP4 codes)
  const int r = L.r, ja = cr * 16 + n16;
  const uint16_t* Ap = (const uint16_t*)L.A + ja;
  const uint32_t* Apf = (const uint32_t*)L.A + ja;   // PF: A is fp32, a 4-byte gather; the raw bits wait in the register
  auto load_step = [&](int kk, sk_wvec(&o)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = kbeg + kk + kg * 8 + i;
      sk_wvec v = {};
      if (!is_xa) {
        if constexpr (FP4) {
          // o[0..3] = row pairs 8 kg + 2 i of the step's block (d_in % 32 == 0 and slabs begin on block boundaries: a block is
          // whole or absent), o[4] = the block's scale bytes of the same 8 columns
          const int k2 = kbeg + kk + kg * 8 + 2 * i;
          if (i < 4) {
            if (col_ok && kk < klen && k2 < d_in) v = sk_load_w((const sk_wvec*)(Wp + (size_t)(k2 >> 1) * wpitch));
          } else if (i == 4) {
            if (col_ok && kk < klen && kbeg + kk < d_in)
              v = sk_load_w((const sk_wvec*)((const char*)L.wexp + (size_t)((kbeg + kk) >> 5) * d_out + col0));
          }
        } else if (col_ok && kk < klen && k < d_in) v = sk_load_w((const sk_wvec*)(Wp + (size_t)k * wpitch));
      } else {
        if constexpr (PF) {
          if (ja < r && kk < klen && k < d_in) v[0] = Apf[(size_t)k * r];
        } else if (ja < r && kk < klen && k < d_in) v[0] = Ap[(size_t)k * r];
      }
      o[i] = v;
    }
  };
#pragma unroll
  for (int p = 0; p < NPF; ++p) load_step(kk0 + p * SK_KQ, d[p]);

  // ---- the slab of x: [rows][KS + pad], zeros for t >= T and k >= d_in ----
  const int xpitch = (KS + SK_XPAD) * 2;   // bytes
  {
    const T* x = (const T*)L.x;
    const int cpr = KS / 8;
    for (int idx = tid; idx < rows * cpr; idx += 256) {
      const int t = idx / cpr, c = idx - t * cpr, k = kbeg + c * 8;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (t < Tn && k < d_in) v = *(const u32x4*)(x + (size_t)t * d_in + k);
      *(u32x4*)(sk_smem + t * xpitch + c * 16) = v;
    }
  }
  __syncthreads();

  f32x4 acc[SK_NCT][RT];
#pragma unroll
  for (int c = 0; c < SK_NCT; ++c)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc[c][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const char* xa0 = sk_smem + n16 * xpitch + kg * 16;
  u32x4 a[RT];
  // one W fragment, built once, against every live row tile
  auto mma = [&](int c, const u32x4& f) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
      if (RT == 4 || rt == 0 || live(rt)) acc[c][rt] = sk_mfma<T>(a[rt], f, acc[c][rt]);   // RT = 4: a dead tile's a[rt] is zeros
  };

  for (int kb = kk0; kb < klen; kb += NPF * SK_KQ) {
#pragma unroll
    for (int p = 0; p < NPF; ++p) {
      const int kk = kb + p * SK_KQ;
      if (kk < klen) {   // uniform per wave
        a[0] = *(const u32x4*)(xa0 + kk * 2);
#pragma unroll
        for (int rt = 1; rt < RT; ++rt) {
          a[rt] = u32x4{0u, 0u, 0u, 0u};
          if (live(rt)) a[rt] = *(const u32x4*)(xa0 + rt * 16 * xpitch + kk * 2);
        }
        if (is_xa) {
          u32x4 f;
#pragma unroll
          for (int m = 0; m < 4; ++m) {
            if constexpr (PF)   // rounded here, at first use: the requests above stay in flight while x is staged
              f[m] = sk_rn_bits<T>(__uint_as_float(d[p][2 * m][0])) | (sk_rn_bits<T>(__uint_as_float(d[p][2 * m + 1][0])) << 16);
            else
              f[m] = d[p][2 * m][0] | (d[p][2 * m + 1][0] << 16);
          }
          mma(0, f);
        } else if constexpr (FP8) {
          // dword wd of a row = columns 4 wd .. 4 wd + 3: the conversion yields two columns of one row, a fragment register
          // wants two rows of one column
#pragma unroll
          for (int wd = 0; wd < 2; ++wd) {
            u32x4 f[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
              const uint32_t r0 = d[p][2 * m][wd], r1 = d[p][2 * m + 1][wd];
              const auto r0l = __builtin_amdgcn_cvt_pk_f32_fp8(r0, false), r0h = __builtin_amdgcn_cvt_pk_f32_fp8(r0, true);
              const auto r1l = __builtin_amdgcn_cvt_pk_f32_fp8(r1, false), r1h = __builtin_amdgcn_cvt_pk_f32_fp8(r1, true);
              f[0][m] = sk_pack_exact<T>(r0l[0], r1l[0]);
              f[1][m] = sk_pack_exact<T>(r0l[1], r1l[1]);
              f[2][m] = sk_pack_exact<T>(r0h[0], r1h[0]);
              f[3][m] = sk_pack_exact<T>(r0h[1], r1h[1]);
            }
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) mma(4 * wd + cc, f[cc]);
          }
        } else if constexpr (FP4) {
          // byte c of a row pair = column c, rows 2 m and 2 m + 1 of the lane's eight: the scaled conversion IS fragment
          // register m of tile c
#pragma unroll
          for (int c = 0; c < SK_NCT; ++c) {
            const float sc = __uint_as_float(((d[p][4][c >> 2] >> (8 * (c & 3))) & 0xffu) << 23);   // E8M0 byte -> 2^e
            u32x4 f;
#pragma unroll
            for (int m = 0; m < 4; ++m) f[m] = cvt_fp4_pair<T>(d[p][m][c >> 2], sc, c & 3);
            mma(c, f);
          }
        } else {
#pragma unroll
          for (int c = 0; c < SK_NCT; ++c) {
            u32x4 f;
#pragma unroll
            for (int m = 0; m < 4; ++m)
              f[m] = __builtin_amdgcn_perm(d[p][2 * m + 1][c >> 1], d[p][2 * m][c >> 1], (c & 1) ? 0x07060302u : 0x05040100u);
            mma(c, f);
          }
        }
        load_step(kk + NPF * SK_KQ, d[p]);   // (requests nothing past the slab)
      }
    }
  }

  // ---- park the four waves' tiles, add them in wave order, store the slab partial ----
  // RT = 4: in two passes of 32 rows (row tiles 0-1, then 2-3), so that the parked tiles of a 128-column range stay under
  // half a CU's LDS; the wave order of every sum is the same
  __syncthreads();   // every wave is done with the x slab: the parked tiles take its place
  float* red = (float*)sk_smem;
  const int prows = RT == 2 ? rows : 32;   // rows a wave parks per pass
#pragma unroll
  for (int ps = 0; ps < RT / 2; ++ps) {
    if (ps) __syncthreads();   // the pass before is read
#pragma unroll
    for (int c = 0; c < SK_NCT; ++c)
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
        if ((2 * ps + hf == 0 || live(2 * ps + hf)) && (c == 0 || !is_xa)) {
#pragma unroll
          for (int q = 0; q < 4; ++q) red[(w * prows + hf * 16 + kg * 4 + q) * SK_RS + c * 16 + n16] = acc[c][2 * ps + hf][q];
        }
    __syncthreads();
    const int t0 = 32 * ps, tn = RT == 2 ? Tn : min(Tn - t0, 32);   // the pass's rows of the call: t0 .. t0 + tn - 1
    if (!is_xa) {
      float* Py = L.Py + ((size_t)s * Tn + t0) * d_out;
      for (int idx = tid; idx < tn * SK_CN; idx += 256) {
        const int t = idx / SK_CN, jc = idx - t * SK_CN;
        const int n = cr * SK_CN + jc;
        // local column jc = n16 * NCT + c sits in fragment c, tile column n16
        const int slot = (jc % SK_NCT) * 16 + jc / SK_NCT;
        float v = red[t * SK_RS + slot];
#pragma unroll
        for (int ww = 1; ww < 4; ++ww) v += red[(ww * prows + t) * SK_RS + slot];
        if (n < d_out) Py[(size_t)t * d_out + n] = v;
      }
    } else {
      // columns 16 cr .. 16 cr + 15 of Ph[s] (columns >= r hold zeros; those past the last tile are never read)
      float* Ph = L.Ph + ((size_t)s * Tn + t0) * 64 + cr * 16;
      for (int idx = tid; idx < tn * 16; idx += 256) {
        const int t = idx >> 4, jj = idx & 15;
        float v = red[t * SK_RS + jj];
#pragma unroll
        for (int ww = 1; ww < 4; ++ww) v += red[(ww * prows + t) * SK_RS + jj];
        Ph[t * 64 + jj] = v;
      }
    }
  }
}

// Phase B: workgroup = 64 columns x 4 token rows, one output element per thread.  Every load a thread needs is independent
// of the others -- its column of B and its bias (cold, from HBM), its slab partials -- so all of them are requested before
// the first is used (at clamped, always valid addresses: no branch stands between the requests): one memory round trip
// instead of a chain of r + 2 S + 1, and only the fp32 additions run in order.
constexpr int SK_BS = 16;   // slab partials requested up front; a layer with more slabs adds the rest in a second loop

// Short batches, data gradient (SH = SK_SH_BWD): the same workgroup over dX -- 64 columns of the layer's d_in x 4 token rows.
// dh = rn(scale * sum_s Ph[s]) goes into LDS and, from the workgroups of the first column block, to memory once per row in the
// layout the chain kernels leave (pad columns zero, 1.0 in column 63 when r <= 63); then per element the Py slabs in slab
// order, the r products dh[t][j] . A[n][j] in order of j (the thread's row of A is contiguous), one rounding, one store.  No bias.
enum SkShort : int { SK_SH_NONE = 0, SK_SH_FWD = 1, SK_SH_BWD = 2 };
template <typename T> __device__ __forceinline__ void skinny_b_tr(const SkGroup& g) {
  __shared__ float hs[4][64];
  int li = 0;
  for (int i = 1; i < g.n; ++i)
    if ((int)blockIdx.x >= g.L[i].startB) li = i;
  const SkLayer& L = g.L[li];
  const int b = (int)blockIdx.x - L.startB;
  const int Tn = L.T, N = L.d_out, r = L.r, S = L.S;
  const int nrg = (Tn + 3) >> 2;
  const int cb = b / nrg, rg = b - cb * nrg;
  const int tid = threadIdx.x, nn = tid & 63, tl = tid >> 6;
  const int t = rg * 4 + tl, n = cb * SK_BN + nn;
  const bool live = t < Tn && n < N;
  const int tc = min(t, Tn - 1), nc = min(n, N - 1), jc = min(nn, r - 1);

  // every request before the first use, at clamped addresses: the thread's row of A (L.B here: [N][r]), its slab partials
  T av[64];
  {
    const T* A = (const T*)L.B + (size_t)nc * r;
#pragma unroll
    for (int j = 0; j < 64; ++j) av[j] = A[min(j, r - 1)];
  }
  float ph[SK_BS], py[SK_BS];
  const float* Ph = L.Ph + (size_t)tc * 64 + jc;
  const size_t phs = (size_t)Tn * 64;
  const float* Py = L.Py + (size_t)tc * N + nc;
  const size_t pys = (size_t)Tn * N;
#pragma unroll
  for (int u = 0; u < SK_BS; ++u) ph[u] = Ph[(size_t)min(u, S - 1) * phs];
#pragma unroll
  for (int u = 0; u < SK_BS; ++u) py[u] = Py[(size_t)min(u, S - 1) * pys];

  {
    float v = 0.f;
#pragma unroll
    for (int u = 0; u < SK_BS; ++u)
      if (u < S) v += ph[u];
    for (int s = SK_BS; s < S; ++s) v += Ph[(size_t)s * phs];
    const float hv = (t < Tn && nn < r) ? to_f32(from_f32<T>(L.scale * v)) : 0.f;
    hs[tl][nn] = hv;
    if (cb == 0 && t < Tn && L.hout) ((T*)L.hout)[(size_t)t * 64 + nn] = from_f32<T>((nn == 63 && r < 64) ? 1.f : hv);
  }
  float acc = 0.f;
#pragma unroll
  for (int u = 0; u < SK_BS; ++u)
    if (u < S) acc += py[u];
  for (int s = SK_BS; s < S; ++s) acc += Py[(size_t)s * pys];
  __syncthreads();
  if (!live) return;
#pragma unroll
  for (int j = 0; j < 64; ++j)
    if (j < r) acc = fmaf(hs[tl][j], to_f32(av[j]), acc);
  ((T*)L.y)[(size_t)t * N + n] = from_f32<T>(acc);
}

// SH: the short-batch forms (factors of T; SK_SH_FWD with either column scaling, SK_SH_BWD plain: the data gradient dequantises in phase A): SK_SH_FWD also stores the h rows it has just rounded, from the workgroups
// of the first column block, in the h_save layout; SK_SH_BWD is the data gradient above
template <typename T, bool FP8 = false, bool PF = false, int SH = SK_SH_NONE> __global__ __launch_bounds__(256) void skinny_b_kernel(const SkGroup g) {
  static_assert(SH == SK_SH_NONE || (!PF && (SH == SK_SH_FWD || !FP8)), "the short-batch forms read factors of T; the data gradient's sums are scaled already");
  if constexpr (SH == SK_SH_BWD) {   // (what follows is dead code in these instantiations)
    skinny_b_tr<T>(g);
    return;
  }
  __shared__ float hs[4][64];
  int li = 0;
  for (int i = 1; i < g.n; ++i)
    if ((int)blockIdx.x >= g.L[i].startB) li = i;
  const SkLayer& L = g.L[li];
  const int b = (int)blockIdx.x - L.startB;
  const int Tn = L.T, d_out = L.d_out, r = L.r, S = L.S;
  const int nrg = (Tn + 3) >> 2;
  const int cb = b / nrg, rg = b - cb * nrg;
  const int tid = threadIdx.x, nn = tid & 63, tl = tid >> 6;
  const int t = rg * 4 + tl, n = cb * SK_BN + nn;
  const bool live = t < Tn && n < d_out;
  const int tc = min(t, Tn - 1), nc = min(n, d_out - 1), jc = min(nn, r - 1);
  const bool dense = L.Py != nullptr;

  // PF: B and the bias are fp32; the loads are requested as they are and each value is rounded once to T where it is used
  typedef typename std::conditional<PF, float, T>::type TP;
  TP bv[64];
  {
    const TP* B = (const TP*)L.B + nc;
#pragma unroll
    for (int j = 0; j < 64; ++j) bv[j] = B[(size_t)min(j, r - 1) * d_out];
  }
  const TP bias = L.bias ? ((const TP*)L.bias)[nc] : from_f32<TP>(0.f);
  int wexp = 0;   // the column's exponent: |e| <= 119, 2^e is a normal fp32 number
  if constexpr (FP8)
    if (dense) wexp = L.wexp[nc];
  float ph[SK_BS], py[SK_BS];
  const float* Ph = L.Ph + (size_t)tc * 64 + jc;
  const size_t phs = (size_t)Tn * 64;
  const float* Py = (dense ? L.Py : L.Ph) + (dense ? (size_t)tc * d_out + nc : 0);   // (never read without W)
  const size_t pys = dense ? (size_t)Tn * d_out : 0;
#pragma unroll
  for (int u = 0; u < SK_BS; ++u) ph[u] = Ph[(size_t)min(u, S - 1) * phs];
#pragma unroll
  for (int u = 0; u < SK_BS; ++u) py[u] = Py[(size_t)min(u, S - 1) * pys];

  // h[t][nn] = rn(scale * sum_s Ph[s][t][nn]), slab order
  {
    float v = 0.f;
#pragma unroll
    for (int u = 0; u < SK_BS; ++u)
      if (u < S) v += ph[u];
    for (int s = SK_BS; s < S; ++s) v += Ph[(size_t)s * phs];
    hs[tl][nn] = (t < Tn && nn < r) ? to_f32(from_f32<T>(L.scale * v)) : 0.f;
    if constexpr (SH == SK_SH_FWD)   // h_save: the rounded row, zeros past r, 1.0 in column 63 when free (the chain kernels' layout)
      if (cb == 0 && t < Tn && L.hout) ((T*)L.hout)[(size_t)t * 64 + nn] = from_f32<T>((nn == 63 && r < 64) ? 1.f : hs[tl][nn]);
  }
  float acc = 0.f;
  if (dense) {
#pragma unroll
    for (int u = 0; u < SK_BS; ++u)
      if (u < S) acc += py[u];
    for (int s = SK_BS; s < S; ++s) acc += Py[(size_t)s * pys];
    if constexpr (FP8) acc *= __uint_as_float((uint32_t)(wexp + 127) << 23);   // sum x . q, scaled once: exact
  }
  __syncthreads();
  if (!live) return;
#pragma unroll
  for (int j = 0; j < 64; ++j)
    if (j < r) acc = fmaf(hs[tl][j], sk_param<T>(bv[j]), acc);
  if (L.bias) acc += sk_param<T>(bias);
  ((T*)L.y)[(size_t)t * d_out + n] = from_f32<T>(acc);
}

size_t skinny_py_bytes(int64_t T, int d_out, int S) { return (size_t)S * (size_t)T * (size_t)d_out * sizeof(float); }
size_t skinny_ph_bytes(int64_t T, int S) { return (size_t)S * (size_t)T * 64 * sizeof(float); }

// ---- 33 <= T <= 64 (sow_forward_skinny_rows): the RT = 4 instantiations of phase A ----
// The slab plan depends on T here.  The x slab is 48 or 64 rows, and two workgroups share a CU's 160 KiB of LDS: the longest
// slab is 768 at T <= 48 (48 x 776 x 2 = 74496 bytes) and 512 above (64 x 520 x 2 = 66560).  The Py partials grow with T
// (S T d_out 4 bytes written and read back), so a layer asks for fewer workgroups than skinny_plan does: DESIGN 4.5d.
#ifndef SOW_SKINNY_ROWS_WANT
#define SOW_SKINNY_ROWS_WANT 512
#endif
#ifndef SOW_SKINNY_ROWS_WANT8
#define SOW_SKINNY_ROWS_WANT8 256
#endif
constexpr int SK_ROWS_MAX = 64;
constexpr int SK_KS_MAX48 = 768, SK_KS_MAX64 = 512;
void skinny_rows_plan(int64_t T, int d_in, int d_out, int acc_kind, int* S, int* KS, int* ncr) {
  if (T <= 32) return skinny_plan(d_in, d_out, acc_kind, S, KS, ncr);   // the plan of sow_forward_skinny, as it is
  const bool codes = acc_is_codes(acc_kind);
  const int nc = acc_kind == SOW_ACC_DENSE || codes ? ceil_div(d_out, sk_cn(codes)) : 0;
  const int want = nc ? ceil_div(codes ? SOW_SKINNY_ROWS_WANT8 : SOW_SKINNY_ROWS_WANT, nc) : 32;
  const int ks_max = T > 48 ? SK_KS_MAX64 : SK_KS_MAX48;
  int ks = ceil_div(ceil_div(d_in, want), SK_KQ) * SK_KQ;
  if (ks < SK_KQ) ks = SK_KQ;
  if (ks > ks_max) ks = ks_max;
  *KS = ks, *S = ceil_div(d_in, ks), *ncr = nc;
}

// the two launches of one (compute dtype, accumulator format, factor dtype, row tiles): one instantiation of each kernel
template <typename T, SkFmt F, bool PF, int RT> static int sk_launch(const SkGroup& g, int na, int nb, size_t lds, hipStream_t stream) {
  constexpr int LDS_X = RT == 2 ? 32 * (SK_KS_MAX + SK_XPAD) * 2 : 48 * (SK_KS_MAX48 + SK_XPAD) * 2;
  static_assert(RT == 2 || 64 * (SK_KS_MAX64 + SK_XPAD) * 2 <= LDS_X, "the 64-row slab is the shorter one");
  constexpr int LDS_PARK = 4 * 32 * sk_rs(F != SK_PLAIN) * 4;   // RT = 4 parks 32 rows per pass
  constexpr int LDS_MAX = LDS_PARK > LDS_X ? LDS_PARK : LDS_X;
  static_assert(RT == 2 || 2 * LDS_MAX <= 160 * 1024, "two workgroups per CU");
  if (lds > (size_t)LDS_MAX) return SOW_ERR_UNSUPPORTED;   // (the plans keep below it)
  SOW_SET_MAX_LDS_ONCE(LDS_MAX, skinny_a_kernel<T, F, PF, RT>);
  hipLaunchKernelGGL((skinny_a_kernel<T, F, PF, RT>), dim3(na), dim3(256), lds, stream, g);
  SOW_CHECK_LAUNCH();
  hipLaunchKernelGGL((skinny_b_kernel<T, F == SK_FP8, PF>), dim3(nb), dim3(256), 0, stream, g);
  SOW_CHECK_LAUNCH();
  return SOW_OK;
}
// every instantiation there is, by [dtype is f16][SkFmt][param_f32][row tiles are 4]
using SkLaunch = int (*)(const SkGroup&, int, int, size_t, hipStream_t);
#define SK_PF_ROW(T, F, PF) {sk_launch<T, F, PF, 2>, sk_launch<T, F, PF, 4>}
#define SK_FMT_ROW(T, F) {SK_PF_ROW(T, F, false), SK_PF_ROW(T, F, true)}
#define SK_DTYPE_ROWS(T) {SK_FMT_ROW(T, SK_PLAIN), SK_FMT_ROW(T, SK_FP8), SK_FMT_ROW(T, SK_FP4)}
static constexpr SkLaunch SK_LAUNCH[2][3][2][2] = {SK_DTYPE_ROWS(bf16_t), SK_DTYPE_ROWS(f16_t)};

// layers: x, W (or nullptr), A, B, bias, y, Py (or nullptr), Ph, T, d_in, d_out, r, scale set by the caller (api.hip has checked
// the admitted set); the plan and the block offsets are filled in here.  param_f32: A, B and bias are fp32.  rows64: every
// layer has 33 <= T <= 64 (skinny_rows_plan, four row tiles); otherwise every layer has T in [1, 32] (skinny_plan, two)
int launch_skinny_fwd(const SkLayer* layers, int n, int dtype, int acc_kind, bool param_f32, hipStream_t stream, bool rows64) {
  if (n <= 0) return SOW_OK;
  if (n > SK_MAXL || (dtype != SOW_BF16 && dtype != SOW_F16)) return SOW_ERR_UNSUPPORTED;
  for (int i = 0; i < n; ++i)
    if (layers[i].T < (rows64 ? 33 : 1) || layers[i].T > (rows64 ? SK_ROWS_MAX : 32)) return SOW_ERR_UNSUPPORTED;
  // the dense layers of a call are of one kind: the kernels are instantiated per kind
  bool codes = false, plain = false;
  for (int i = 0; i < n; ++i) (layers[i].wexp ? codes : plain) |= layers[i].W != nullptr;
  if ((codes && plain) || (!acc_is_codes(acc_kind) && codes) || (acc_is_codes(acc_kind) && plain)) return SOW_ERR_UNSUPPORTED;
  const SkFmt fmt = codes ? sk_fmt(acc_kind) : SK_PLAIN;
  const int SK_RS = sk_rs(codes);
  SkGroup g;
  g.n = n;
  int na = 0, nb = 0;
  size_t lds = 0;
  for (int i = 0; i < n; ++i) {
    SkLayer& L = g.L[i];
    L = layers[i];
    if (!L.W) L.wexp = nullptr;
    int ncr;
    skinny_rows_plan(L.T, L.d_in, L.d_out, !L.W ? SOW_ACC_NONE : codes ? acc_kind : SOW_ACC_DENSE, &L.S, &L.KS, &ncr);
    L.ncr = ncr;
    L.startA = na, L.startB = nb;
    na += L.S * ((L.r + 15) / 16 + ncr);
    nb += ceil_div(L.d_out, SK_BN) * ((L.T + 3) / 4);
    const int rows = rows64 ? (L.T > 48 ? 64 : 48) : (L.T > 16 ? 32 : 16);
    const size_t xb = (size_t)rows * (L.KS + SK_XPAD) * 2, rb = (size_t)4 * (rows64 ? 32 : rows) * SK_RS * sizeof(float);
    lds = xb > lds ? xb : lds;
    lds = rb > lds ? rb : lds;
  }
  // MXFP4: the scale went into the conversion, Py holds sum x . W^ and phase B is the plain one
  return SK_LAUNCH[dtype == SOW_F16][fmt][param_f32][rows64](g, na, nb, lds, stream);
}

// ---- short batches: 1 <= T <= SK_SHORT_MAX rows of a dense-accumulator layer, forward and data gradient ----
// A layer is ceil(T / 64) row blocks on one W, every block an entry of the group with its own x / y / Py / Ph / hout.  The plan
// counts the blocks: about SK_SHORT_WANT workgroups over blocks x column ranges x slabs, not per block -- the slab partials are S T N
// floats written and read back, and sixteen blocks fill the chip without short slabs.  Slabs are at most 512 (the 64-row x slab:
// two workgroups per CU) and whole rounds of the four waves (kq).  All blocks of a layer take the one plan, and a block of fewer
// than 49 rows pads with a zero tile: the order of a row's sum does not depend on the block it is in or on its place there.
#ifndef SOW_SKINNY_SHORT_WANT
#define SOW_SKINNY_SHORT_WANT 512
#endif
void short_rows_plan(int64_t T, int K, int N, int kq, int* S, int* KS, int* ncr) {
  const int nblk = (int)ceil_div(T, (int64_t)SK_ROWS_MAX), nc = ceil_div(N, sk_cn(false));
  const int want = ceil_div(SOW_SKINNY_SHORT_WANT, nc * (nblk > 0 ? nblk : 1));
  int ks = ceil_div(ceil_div(K, want), kq) * kq;
  if (ks < kq) ks = kq;
  if (ks > SK_KS_MAX64) ks = SK_KS_MAX64;
  *KS = ks, *S = ceil_div(K, ks), *ncr = nc;
}

// ... of the forward on codes (sow_forward_short_codes): the RT = 4 code forms of phase A have 128-column ranges and run one workgroup per
// CU, so the count is SOW_SKINNY_SHORT_WANT8 workgroups over blocks x 128-column ranges x slabs.  Slabs are whole rounds of
// the four waves (128: whole MX blocks too) and at most 512, the 64-row x slab of those forms.
#ifndef SOW_SKINNY_SHORT_WANT8
#define SOW_SKINNY_SHORT_WANT8 256
#endif
void short_codes_plan(int64_t T, int K, int N, int* S, int* KS, int* ncr) {
  const int nblk = (int)ceil_div(T, (int64_t)SK_ROWS_MAX), nc = ceil_div(N, sk_cn(true));
  const int want = ceil_div(SOW_SKINNY_SHORT_WANT8, nc * (nblk > 0 ? nblk : 1));
  int ks = ceil_div(ceil_div(K, want), SK_SHORT_KQ_FWD) * SK_SHORT_KQ_FWD;
  if (ks < SK_SHORT_KQ_FWD) ks = SK_SHORT_KQ_FWD;
  if (ks > SK_KS_MAX64) ks = SK_KS_MAX64;
  *KS = ks, *S = ceil_div(K, ks), *ncr = nc;
}

// F: the format W is stored in.  Forward: phase A is the RT = 4 form of F as sow_forward_skinny_rows launches it, phase B SK_SH_FWD with
// the E4M3 column scaling where F asks for it.  Data gradient: the TR form of F, and the plain SK_SH_BWD (the sums are scaled)
template <typename T, SkFmt F, bool BWD> static int sk_launch_short(const SkGroup& g, int na, int nb, size_t lds, hipStream_t stream) {
  // (the forward's phase A is the RT = 4 form of sow_forward_skinny_rows itself: the same limit as sk_launch sets for it)
  constexpr int LDS_MAX = 48 * (SK_KS_MAX48 + SK_XPAD) * 2;
  constexpr int LDS_PARK = 4 * 32 * sk_rs(F != SK_PLAIN && !BWD) * 4;
  static_assert(64 * (SK_KS_MAX64 + SK_XPAD) * 2 <= LDS_MAX && LDS_PARK <= LDS_MAX && 2 * LDS_MAX <= 160 * 1024, "two workgroups per CU");
  if (lds > (size_t)LDS_MAX) return SOW_ERR_UNSUPPORTED;
  SOW_SET_MAX_LDS_ONCE(LDS_MAX, skinny_a_kernel<T, F, false, 4, BWD>);
  hipLaunchKernelGGL((skinny_a_kernel<T, F, false, 4, BWD>), dim3(na), dim3(256), lds, stream, g);
  SOW_CHECK_LAUNCH();
  hipLaunchKernelGGL((skinny_b_kernel<T, F == SK_FP8 && !BWD, false, BWD ? SK_SH_BWD : SK_SH_FWD>), dim3(nb), dim3(256), 0, stream, g);
  SOW_CHECK_LAUNCH();
  return SOW_OK;
}
// by [dtype is f16][SkFmt][bwd]
#define SK_SHORT_ROW(T, F) {sk_launch_short<T, F, false>, sk_launch_short<T, F, true>}
#define SK_SHORT_ROWS(T) {SK_SHORT_ROW(T, SK_PLAIN), SK_SHORT_ROW(T, SK_FP8), SK_SHORT_ROW(T, SK_FP4)}
static constexpr SkLaunch SK_LAUNCH_SHORT[2][3][2] = {SK_SHORT_ROWS(bf16_t), SK_SHORT_ROWS(f16_t)};

int launch_skinny_short(const SkLayer* entries, int n, int dtype, bool bwd, hipStream_t stream, int acc_kind) {
  if (n <= 0) return SOW_OK;
  if ((dtype != SOW_BF16 && dtype != SOW_F16) || (acc_kind != SOW_ACC_DENSE && !acc_is_codes(acc_kind))) return SOW_ERR_UNSUPPORTED;
  const bool codes = acc_is_codes(acc_kind);
  const bool wide = codes && !bwd;   // 128-column ranges: the forward on codes alone
  const int kq = bwd ? SK_SHORT_KQ_BWD : SK_SHORT_KQ_FWD;
  for (int i = 0; i < n; ++i) {
    const SkLayer& E = entries[i];
    if (E.T < 1 || E.T > SK_ROWS_MAX || !E.W || !E.Py || !E.Ph || E.r < 1 || E.r > 64 || E.KS < kq || E.KS > SK_KS_MAX64 || E.KS % kq ||
        E.S != ceil_div(E.d_in, E.KS) || E.ncr != ceil_div(E.d_out, sk_cn(wide)) || codes != (E.wexp != nullptr))
      return SOW_ERR_UNSUPPORTED;
    // MXFP4 blocks are whole along the layer's d_in: the forward's contraction, the data gradient's output
    if (acc_kind == SOW_ACC_DENSE_FP4 && (bwd ? E.d_out : E.d_in) % 32) return SOW_ERR_UNSUPPORTED;
  }
  for (int i0 = 0; i0 < n; i0 += SK_MAXL) {
    SkGroup g;
    g.n = n - i0 < SK_MAXL ? n - i0 : SK_MAXL;
    int na = 0, nb = 0;
    size_t lds = (size_t)4 * 32 * sk_rs(wide) * sizeof(float);
    for (int i = 0; i < g.n; ++i) {
      SkLayer& L = g.L[i];
      L = entries[i0 + i];
      L.startA = na, L.startB = nb;
      na += L.S * ((L.r + 15) / 16 + L.ncr);
      nb += ceil_div(L.d_out, SK_BN) * ((L.T + 3) / 4);
      const size_t xb = (size_t)(L.T > 48 ? 64 : 48) * (L.KS + SK_XPAD) * 2;
      lds = xb > lds ? xb : lds;
    }
    const int rc = SK_LAUNCH_SHORT[dtype == SOW_F16][sk_fmt(acc_kind)][bwd](g, na, nb, lds, stream);
    if (rc) return rc;
  }
  return SOW_OK;
}

}  // namespace sow
