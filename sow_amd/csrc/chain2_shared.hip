// Shared-input form of the bf16 / f16 streaming chain (chain2.hip): n <= 4 sibling layers on ONE input, one launch.
//
//   forward :  y_i  = (scale_i * x . A_i) . B_i + bias_i           for i < n          (x read once)
//   backward:  dh_i = scale_i * dY_i . B_i^T  (into each layer's dh region, [T, 64], exactly as chain2 writes it)
//              dX   = grad_beta * dX + sum_i dh_i . A_i^T          (one fp32 sum, rounded once; nothing else writes dX)
//
// Every workgroup owns a 64-token block for EVERY sibling and runs chain2's wave layout (4 compute waves = 2 token groups x 2
// halves, 2 loader waves), X ring, factor ring, hand-off and epilogue unchanged; what changes is the order of the chunks:
//   forward : phase 1 walks the K stages of x once; after the barrier of stage st the compute waves read the X stage into
//             registers ONCE and contract it with the A_i chunk st of every sibling (chunks st*n + i, one barrier each).  All
//             n H^T accumulators are live through phase 1 (16 VGPRs each).  Then, sibling by sibling: hand-off (scale, mask,
//             round, h_save_i, exchange of the rank tiles) and phase 2 over B_i with sibling i's epilogue.
//   backward: sibling by sibling, phase 1 streams dY_i against B_i and hands dh_i off (kept packed in registers, 16 VGPRs
//             each); phase 2 walks the 64-column slices of dX, contracting dh_i with the A_i chunk of the slice for every i
//             into ONE fp32 accumulator, then parks and stores the slice once.
// Each accumulator sees the same X stage, the same factor chunk and the same k order as in chain2, so y_i, h_save_i and dh_i
// are bit-identical to sow_forward_group / sow_backward_group(BWD_DATA); dX is the one new result.
//
// LDS: chain2's 80 KiB (two workgroups per CU): 6 x 8 KiB factor chunk slots (5 ahead) + 2 token groups x 4 x 4 KiB X
// stages.  n chunks per K stage is the pressure point: the factor ring is not widened (that would cost the second workgroup
// per CU), the loaders stay 5 CHUNKS ahead, i.e. 5 / n stages.  The A chunks are re-read from L2 (a 512 x 50 A is 51 KB).
#include "kernels.hpp"
#include "lds_dma.hpp"

namespace sow {

constexpr int CS_NTG = 2;            // token groups (32 tokens) per workgroup
constexpr int CS_NCW = 2 * CS_NTG;   // compute waves
constexpr int CS_NLW = 2;            // loader waves
constexpr int CS_BM = 32 * CS_NTG;   // tokens per workgroup
constexpr int CS_DEPTH = 4;          // X stage slots per token group (3 in flight)
constexpr int CS_STAGE = 4096;       // [32 tok][64 k] 16-bit
constexpr int CS_NSLOT = 6;          // factor chunk slots
constexpr int CS_AHEAD = 5;          // chunks the loaders run ahead
constexpr int CS_FSLOT = 8192;       // [64][64] 16-bit
constexpr int CS_LPW = 8 / CS_NLW;   // 1-KiB DMA instructions per loader wave per chunk
constexpr int CS_RING0 = CS_NSLOT * CS_FSLOT;
constexpr int CS_RING = CS_DEPTH * CS_STAGE;            // 16 KiB per token group: two 8-KiB fp32 park tiles
constexpr int CS_LDS = CS_RING0 + CS_NTG * CS_RING;     // 80 KiB
constexpr int CS_THREADS = 64 * (CS_NCW + CS_NLW);
constexpr int CS_RESIDENT = 512;
static_assert(CS_LDS == 80 * 1024 && CS_NSLOT == CS_AHEAD + 1, "80 KiB: two workgroups per CU");

template <bool TR> __device__ __forceinline__ int cs_img_chunk(int row, int c) {
  return TR ? (c ^ (((row >> 1) & 1) << 2)) : (c ^ ((row >> 1) & 7));
}

// Chunk schedule (both the loaders and the compute waves follow it; one raw barrier per chunk plus `extra` barriers in front
// of some chunks, as in chain2, where the hand-off barrier sits in front of the first phase-2 chunk):
//   forward : [A_0 st0, .., A_{n-1} st0, A_0 st1, ...]  [B_0 sl0 .. B_0 sl_last] [B_1 ...] ...
//             extra: 1 before B_0 sl0 (hand-off 0); 3 before B_i sl0, i > 0 (last slice parked, end, hand-off i); 2 at the end
//   backward: [B_0 st0 .. B_0 st_last] [B_1 ...] ... [A_0 sl0, .., A_{n-1} sl0, A_0 sl1, ...]
//             extra: 2 before B_i st0, i > 0 (hand-off i-1, exchange slot free); 1 before A_0 sl0 (hand-off n-1); 2 at the end
struct CsChunk {
  int sib, ci, is_a, extra;
};
// chunk count of sibling i's own run: forward, the slices of B_i; backward, the stages of B_i
template <bool BWD> __device__ __forceinline__ int cs_run(const ChainGroup& g, int i) { return ((BWD ? g.p[i].D1 : g.p[i].D2) + 63) / 64; }
template <bool BWD, int N> __device__ __forceinline__ CsChunk cs_chunk(const ChainGroup& g, int c, int nst_f) {
  CsChunk k{0, 0, 0, 0};
  if constexpr (!BWD) {
    const int p1 = N * nst_f;
    if (c < p1) {
      k.sib = c % N, k.ci = c / N, k.is_a = 1;
      return k;
    }
    int cc = c - p1;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if (k.sib == i && cc >= cs_run<BWD>(g, i)) cc -= cs_run<BWD>(g, i), k.sib = i + 1;
    }
    k.ci = cc;
    if (cc == 0) k.extra = k.sib == 0 ? 1 : 3;
  } else {
    int p1 = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) p1 += cs_run<BWD>(g, i);
    if (c >= p1) {
      const int cc = c - p1;
      k.sib = cc % N, k.ci = cc / N, k.is_a = 1;
      if (cc == 0) k.extra = 1;
      return k;
    }
    int cc = c;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if (k.sib == i && cc >= cs_run<BWD>(g, i)) cc -= cs_run<BWD>(g, i), k.sib = i + 1;
    }
    k.ci = cc;
    if (cc == 0 && k.sib > 0) k.extra = 2;
  }
  return k;
}

template <typename T, bool BWD, bool P16, int N>
__device__ __forceinline__ void chain2_shared_block(const ChainGroup& g, const int tb, char* smem, const int t, int lane,
                                                    const int w) {
  constexpr bool TR = !BWD;
  const int64_t m0 = (int64_t)tb * CS_BM;
  const int64_t M = g.p[0].M;
  // forward: the shared K (= d_in) and per-sibling slices; backward: per-sibling stages and the shared d_in slices
  const int nst_f = BWD ? 0 : (g.p[0].D1 + 63) / 64;
  const int nsl_b = BWD ? (g.p[0].D2 + 63) / 64 : 0;
  int total = BWD ? N * nsl_b : N * nst_f;
#pragma unroll
  for (int i = 0; i < N; ++i) total += cs_run<BWD>(g, i);
  const char* zp = zero_page_for(lane);

  if (w >= CS_NCW) {
    // ------------------------------------------------------------------ loader waves
    __builtin_amdgcn_s_setprio(3);
    const int lw = w - CS_NCW;
    // A is [d_in, r_i] for every sibling in both directions: the last-row fix-up belongs to the same loader wave for all
    const int rows_a = BWD ? g.p[0].D2 : g.p[0].D1;
    const bool own_last = rows_a > 0 && lw == ((rows_a - 1) & 63) / (8 * CS_LPW);
    uint32_t last_row_dw[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const T* Ai = (const T*)(BWD ? g.p[i].F2b : g.p[i].F1b);
      last_row_dw[i] = 0u;
      if (own_last && lane < 32 && 2 * lane < g.p[i].rb) last_row_dw[i] = *((const uint32_t*)(Ai + (int64_t)(rows_a - 1) * g.p[i].rb) + lane);
      asm volatile("" : "+v"(last_row_dw[i]));
    }
    auto issue = [&](int c) {
      const CsChunk k = cs_chunk<BWD, N>(g, c, nst_f);
      const ChainParams& p = g.p[k.sib];
      char* slot = smem + (c % CS_NSLOT) * CS_FSLOT;
      if (k.is_a) {
        const T* Amat = (const T*)(BWD ? p.F2b : p.F1b);
        const char* a_end = (const char*)(Amat + (int64_t)rows_a * p.rb);
#pragma unroll
        for (int ii = 0; ii < CS_LPW; ++ii) {
          const int row = 8 * (CS_LPW * lw + ii) + (lane >> 3);
          const char* q = (const char*)(Amat + (int64_t)row * p.rb) + 16 * cs_img_chunk<TR>(row, lane & 7) + (int64_t)k.ci * 128 * p.rb;
          dma16(q + 16 <= a_end ? (const void*)q : (const void*)zp, slot + (CS_LPW * lw + ii) * 1024);
        }
      } else {
        const T* Bmat = (const T*)(BWD ? p.F1b : p.F2b);
        const int64_t ldb = BWD ? p.ldf1b : p.ldf2b;
        const int cols_b = BWD ? p.D1 : p.D2;
#pragma unroll
        for (int ii = 0; ii < CS_LPW; ++ii) {
          const int row = 8 * (CS_LPW * lw + ii) + (lane >> 3);
          const int lc = cs_img_chunk<TR>(row, lane & 7);
          const char* q = (row < p.rb && k.ci * 64 + 8 * lc < cols_b) ? (const char*)(Bmat + (int64_t)row * ldb + 8 * lc + k.ci * 64) : zp;
          dma16((const void*)q, slot + (CS_LPW * lw + ii) * 1024);
        }
      }
    };
    const int p1_end = BWD ? total - N * nsl_b : N * nst_f;   // first phase-2 chunk
    const int pre = total < CS_AHEAD ? total : CS_AHEAD;
    for (int c = 0; c < pre; ++c) issue(c);
    for (int c = 0; c < total; ++c) {
      const int newer = (total - 1 - c) < (CS_AHEAD - 1) ? (total - 1 - c) : (CS_AHEAD - 1);
      wait_groups<CS_LPW>(newer);
      const CsChunk k = cs_chunk<BWD, N>(g, c, nst_f);
      if (k.is_a) {   // fix-up: rewrite the last row of A (its DMA pieces past the end of the buffer were zero-filled)
        const int lr = rows_a - 1 - k.ci * 64;
        if (own_last && lr >= 0 && lr < 64 && lane < 32) {
          uint32_t v = 0u;
#pragma unroll
          for (int i = 0; i < N; ++i)
            if (k.sib == i) v = last_row_dw[i];
          *(uint32_t*)(smem + (c % CS_NSLOT) * CS_FSLOT + lr * 128 + cs_img_chunk<TR>(lr, lane >> 2) * 16 + (lane & 3) * 4) = v;
        }
      }
      if (c == p1_end) __builtin_amdgcn_s_setprio(0);
      for (int e = 0; e < k.extra; ++e) raw_barrier();
      raw_barrier();   // chunk c visible to the consumers; they have finished chunk c-1
      if (c + CS_AHEAD < total) issue(c + CS_AHEAD);
    }
    raw_barrier();   // last slice parked
    raw_barrier();   // end of block
    return;
  }

  // -------------------------------------------------------------------- compute waves
  const int tg = w & 1, hh = w >> 1;
  int li = lane & 31, lh = lane >> 5;
  const int gq = lane >> 4, jj = lane & 15, q = jj >> 2, pp = jj & 3;
  const int h2 = gq >> 1;
  char* ring = smem + CS_RING0 + tg * CS_RING;
  const uint32_t ring_a = lds_addr(ring);
  const uint32_t slot_a = lds_addr(smem);
  const int64_t tok0 = m0 + 32 * tg;
  const int64_t tok = tok0 + li;
  uint32_t xoff = (uint32_t)(li * 128);
  int xsw = (li >> 1) & 7;
  int drow = lane >> 3, dpc = lane & 7;
  uint32_t foff1, foff2;
  if constexpr (TR) {
    const int col = hh * 32 + 16 * (gq & 1) + 4 * pp;
    const int r1 = 8 * h2 + q, r2 = 4 * h2 + q;
    foff1 = (uint32_t)(r1 * 128 + cs_img_chunk<true>(r1, col >> 3) * 16 + (col & 7) * 2);
    foff2 = (uint32_t)(r2 * 128 + cs_img_chunk<true>(r2, col >> 3) * 16 + (col & 7) * 2);
  } else {
    foff1 = (uint32_t)((hh * 32 + li) * 128);
    foff2 = (uint32_t)((hh * 32 + li) * 128 + 8 * lh);
  }
  int chunk = 0;   // chunk counter: the factor slot of the next barrier is chunk % NSLOT
  // Opaque per loop iteration (as chain2_kernel does per block): the per-lane LDS / global address arithmetic of an iteration
  // is recomputed inside it.  Hoisted out of the loops it stays live across the whole block, and with the 16 VGPRs per sibling
  // of H / dh the 3- and 4-sibling forms would spill.
  auto refresh = [&]() {
    asm volatile("" : "+v"(lane), "+v"(li), "+v"(lh), "+v"(xoff), "+v"(xsw), "+v"(drow), "+v"(dpc), "+v"(foff1), "+v"(foff2));
  };

  // X stage DMA of one phase-1 run (X, ldx, D1): this wave issues rows 16 hh .. 16 hh + 15 of every stage; per-lane source
  // pointers of stage 0, advanced by 128 bytes per stage (rows past M read the zero page), as in chain2
  struct XSrc {
    const char* src[2];
    int stride[2], lc[2];
  };
  auto x_sources = [&](const ChainParams& p) {
    XSrc xs;
#pragma unroll
    for (int ii = 0; ii < 2; ++ii) {
      const int row = 8 * (2 * hh + ii) + drow;
      const int lc = dpc ^ ((row >> 1) & 7);
      const int64_t tk = tok0 + row;
      const bool v = tk < M;
      xs.src[ii] = v ? (const char*)((const T*)p.X + tk * p.ldx + lc * 8) : zp;
      xs.stride[ii] = v ? 128 : 0;
      xs.lc[ii] = lc;
    }
    return xs;
  };
  auto issue_x = [&](const ChainParams& p, const XSrc& xs, int st) {
    char* dst = ring + (st % CS_DEPTH) * CS_STAGE;
#pragma unroll
    for (int ii = 0; ii < 2; ++ii) {
      const char* qq = xs.src[ii] + st * xs.stride[ii];
      if (st * 64 + xs.lc[ii] * 8 >= p.D1) qq = zp;
      if (p.nt_load) dma16_nt((const void*)qq, dst + (2 * hh + ii) * 1024);
      else dma16((const void*)qq, dst + (2 * hh + ii) * 1024);
    }
  };
  // one 64-row factor chunk, phase-1 geometry: ff[ks] = rank tile hh, k-steps 0..3
  auto read_f1 = [&](uint32_t fs, u32x4* ff) {
    if constexpr (TR) {
      u32x2 bl[4], bh[4];
      const uint32_t b0 = fs + foff1;
      DS_READ_TR(bl[0], b0, 0);
      DS_READ_TR(bh[0], b0, 512);
      DS_READ_TR(bl[1], b0, 2048);
      DS_READ_TR(bh[1], b0, 2048 + 512);
      DS_READ_TR(bl[2], b0, 4096);
      DS_READ_TR(bh[2], b0, 4096 + 512);
      DS_READ_TR(bl[3], b0, 6144);
      DS_READ_TR(bh[3], b0, 6144 + 512);
      LGKM_WAIT0();
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) ff[ks] = join2(bl[ks], bh[ks]);
    } else {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) DS_READ_B128(ff[ks], fs + foff1 + (uint32_t)(((2 * ks + lh) ^ xsw) * 16), 0);
      LGKM_WAIT0();
    }
  };
  // phase-2 geometry: the A-side operand of one output slice
  auto read_f2 = [&](uint32_t fs, u32x2* bl, u32x2* bh) {
    if constexpr (TR) {
      DS_READ_TR(bl[0], fs, 0);
      DS_READ_TR(bh[0], fs, 1024);
      DS_READ_TR(bl[1], fs, 2048);
      DS_READ_TR(bh[1], fs, 2048 + 1024);
      DS_READ_TR(bl[2], fs, 4096);
      DS_READ_TR(bh[2], fs, 4096 + 1024);
      DS_READ_TR(bl[3], fs, 6144);
      DS_READ_TR(bh[3], fs, 6144 + 1024);
    } else {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        DS_READ_B64(bl[ks], fs + (uint32_t)(((2 * ks) ^ xsw) * 16), 0);
        DS_READ_B64(bh[ks], fs + (uint32_t)(((2 * ks + 1) ^ xsw) * 16), 0);
      }
    }
    LGKM_WAIT0();
  };
  // hand-off, first half: scale, mask rank rows >= r, round; h_save (with 1.0 in column 63 when free) -> own[2]
  auto finish_h = [&](const ChainParams& p, const f32x16& hacc, u32x4* own) {
    float hv[16];
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int r = hh * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
      hv[reg] = r < p.rb ? hacc[reg] * p.scale : 0.f;
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
      own[a] = (u32x4){pack16x2<T>(hv[8 * a + 0], hv[8 * a + 1]), pack16x2<T>(hv[8 * a + 2], hv[8 * a + 3]),
                       pack16x2<T>(hv[8 * a + 4], hv[8 * a + 5]), pack16x2<T>(hv[8 * a + 6], hv[8 * a + 7])};
    if (p.Hsave && tok < M) {
      T* Hs = (T*)p.Hsave + tok * 64 + hh * 32 + 4 * lh;
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        u32x2 v = {pack16x2<T>(hv[4 * rq + 0], hv[4 * rq + 1]), pack16x2<T>(hv[4 * rq + 2], hv[4 * rq + 3])};
        if (hh == 1 && rq == 3 && lh == 1 && p.rb < 64) v[1] = (v[1] & 0xffffu) | (DT<T>::one_bits << 16);
        *(u32x2*)(Hs + 8 * rq) = v;
      }
    }
  };
  // hand-off, second half: exchange the two rank tiles of the token group through X slot `xs` (one barrier)
  auto exchange = [&](int xs, const u32x4* own, u32x4* hf) {
    char* xch = ring + xs * CS_STAGE;
    *(u32x4*)(xch + hh * 2048 + lane * 16) = own[0];
    *(u32x4*)(xch + hh * 2048 + 1024 + lane * 16) = own[1];
    raw_barrier();
    u32x4 oth[2];
    const uint32_t pa = ring_a + (uint32_t)(xs * CS_STAGE + (hh ^ 1) * 2048 + lane * 16);
    DS_READ_B128(oth[0], pa, 0);
    DS_READ_B128(oth[1], pa, 1024);
    LGKM_WAIT0();
    hf[0] = hh ? oth[0] : own[0], hf[1] = hh ? oth[1] : own[1];
    hf[2] = hh ? own[0] : oth[0], hf[3] = hh ? own[1] : oth[1];
  };

  // ---- epilogue of one output slice (chain2's): fp32 park tiles [32 tok][64 col] (2 buffers of 8 KiB) or, with P16 (no
  // bias, beta = 0: the stored value is exactly T(acc)), 16-bit park tiles in ring slots 1..3 and 256-byte pair stores
  auto tile_addr = [&](int buf, int row, int ch) { return ring_a + (uint32_t)(buf * 8192 + row * 256 + ((ch ^ (row & 15)) * 16)); };
  auto flush = [&](const ChainParams& p, int sl_prev) {
    T* Y = (T*)p.Y;
    const T* bias = (const T*)p.bias;
    const int buf = sl_prev & 1;
    u32x4 v0[2], v1[2];
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int r = 16 * hh + pass * 8 + (lane >> 3), c8 = lane & 7;
      DS_READ_B128(v0[pass], tile_addr(buf, r, 2 * c8), 0);
      DS_READ_B128(v1[pass], tile_addr(buf, r, 2 * c8 + 1), 0);
    }
    LGKM_WAIT0();
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int r = 16 * hh + pass * 8 + (lane >> 3), c8 = lane & 7;
      const int64_t tk = tok0 + r;
      const int col = sl_prev * 64 + c8 * 8;
      if (tk < M && col < p.D2) {
        float v[8];
        const float* f0 = (const float*)&v0[pass];
        const float* f1 = (const float*)&v1[pass];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = f0[e], v[4 + e] = f1[e];
        T* dst = Y + tk * p.ldy + col;
        if (p.beta != 0.f) {
          const u32x4 old = *(const u32x4*)dst;
          const T* o = (const T*)&old;
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] += p.beta * (float)o[e];
        }
        if (bias) {
          const u32x4 bv = *(const u32x4*)(bias + col);
          const T* bb = (const T*)&bv;
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] += (float)bb[e];
        }
        const u32x4 ov = {pack16x2<T>(v[0], v[1]), pack16x2<T>(v[2], v[3]), pack16x2<T>(v[4], v[5]), pack16x2<T>(v[6], v[7])};
        if (p.nt_store) asm volatile("global_store_dwordx4 %0, %1, off nt" ::"v"(dst), "v"(ov) : "memory");
        else *(u32x4*)dst = ov;
      }
    }
  };
  auto tile16_addr = [&](int buf, int row, int ch) {
    return ring_a + (uint32_t)((CS_DEPTH - 3) * CS_STAGE + buf * 4096 + row * 128 + ((ch ^ ((row >> 1) & 7)) * 16));
  };
  auto store16 = [&](const ChainParams& p, int r, int col, u32x4 ov) {
    const int64_t tk = tok0 + r;
    if (tk < M && col < p.D2) {
      T* dst = (T*)p.Y + tk * p.ldy + col;
      if (p.nt_store) asm volatile("global_store_dwordx4 %0, %1, off nt" ::"v"(dst), "v"(ov) : "memory");
      else *(u32x4*)dst = ov;
    }
  };
  auto flush16 = [&](const ChainParams& p, int sl_prev) {
    u32x4 v[2];
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) DS_READ_B128(v[pass], tile16_addr(sl_prev % 3, 16 * hh + pass * 8 + (lane >> 3), lane & 7), 0);
    LGKM_WAIT0();
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) store16(p, 16 * hh + pass * 8 + (lane >> 3), sl_prev * 64 + (lane & 7) * 8, v[pass]);
  };
  auto flush_pair16 = [&](const ChainParams& p, int sl_a) {
    u32x4 v[4];
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const int r = 16 * hh + ps * 4 + (lane >> 4), c16 = lane & 15;
      DS_READ_B128(v[ps], tile16_addr((sl_a + (c16 >> 3)) % 3, r, c16 & 7), 0);
    }
    LGKM_WAIT0();
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) store16(p, 16 * hh + ps * 4 + (lane >> 4), sl_a * 64 + (lane & 15) * 8, v[ps]);
  };
  // after the MFMAs of slice sl: store earlier slices while this slice's MFMAs drain, then park this one (chain2's order).  The
  // data gradient parks first: that frees the accumulator before the store path loads its 16 VGPRs, which the 4-sibling
  // form (64 VGPRs of dh live) needs to stay out of scratch.  The tiles differ either way: sl % 3 against (sl - 2, sl - 1) %
  // 3, sl & 1 against (sl - 1) & 1.
  constexpr bool park_first = BWD;
  auto park = [&](int sl, const f32x16& yacc) {
    if constexpr (P16) {
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const u32x2 v = {pack16x2<T>(yacc[4 * rq + 0], yacc[4 * rq + 1]), pack16x2<T>(yacc[4 * rq + 2], yacc[4 * rq + 3])};
        *(u32x2*)(ring + (CS_DEPTH - 3) * CS_STAGE + (sl % 3) * 4096 + li * 128 + (((hh * 4 + rq) ^ ((li >> 1) & 7)) * 16) + lh * 8) = v;
      }
    } else {
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const int ch = hh * 8 + 2 * rq + lh;
        f32x4 v = {yacc[4 * rq + 0], yacc[4 * rq + 1], yacc[4 * rq + 2], yacc[4 * rq + 3]};
        *(f32x4*)(ring + (sl & 1) * 8192 + li * 256 + ((ch ^ (li & 15)) * 16)) = v;
      }
    }
  };
  auto store_earlier = [&](const ChainParams& p, int sl) {
    if constexpr (P16) {
      if (sl >= 2 && !(sl & 1)) flush_pair16(p, sl - 2);
    } else {
      if (sl > 0) flush(p, sl - 1);
    }
  };
  auto epilogue = [&](const ChainParams& p, int sl, const f32x16& yacc) {
    if constexpr (park_first) {
      park(sl, yacc);
      store_earlier(p, sl);
    } else {
      store_earlier(p, sl);
      park(sl, yacc);
    }
  };
  // after the last slice: the partner has parked it; store what is left; end barrier (the rings may be overwritten)
  auto finish_slices = [&](const ChainParams& p, int nsl) {
    raw_barrier();
    if constexpr (P16) {
      if (nsl >= 2 && !(nsl & 1)) flush_pair16(p, nsl - 2);
      else flush16(p, nsl - 1);
    } else {
      flush(p, nsl - 1);
    }
    raw_barrier();
  };
  // this lane's row of one X stage, the phase-1 MFMA operand of every factor chunk of the stage
  auto read_x_stage = [&](uint32_t xs, u32x4* xf) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) DS_READ_B128(xf[ks], xs + (uint32_t)(((2 * ks + lh) ^ xsw) * 16), 0);
  };

  if constexpr (!BWD) {
    // ================================================================== forward
    const ChainParams& p0 = g.p[0];
    f32x16 hacc[N];
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) hacc[i][r] = 0.f;
    const int nst = nst_f;
    const int pre = nst < (CS_DEPTH - 1) ? nst : (CS_DEPTH - 1);
    const XSrc xs0 = x_sources(p0);
    for (int st = 0; st < pre; ++st) issue_x(p0, xs0, st);
#pragma unroll 1
    for (int st = 0; st < nst; ++st) {
      refresh();
      const int newer = (nst - 1 - st) < (CS_DEPTH - 2) ? (nst - 1 - st) : (CS_DEPTH - 2);
      wait_groups<2>(newer);
      raw_barrier();   // X stage st (both halves) and A_0 chunk st
      if (st + CS_DEPTH - 1 < nst) issue_x(p0, xs0, st + CS_DEPTH - 1);
      u32x4 xf[4];
      read_x_stage(ring_a + (uint32_t)((st % CS_DEPTH) * CS_STAGE) + xoff, xf);
#pragma unroll
      for (int i = 0; i < N; ++i) {
        if (i > 0) raw_barrier();   // A_i chunk st
        u32x4 ff[4];
        read_f1(slot_a + (uint32_t)((chunk % CS_NSLOT) * CS_FSLOT), ff);
        ++chunk;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) hacc[i] = mfma32(as_v8<T>(ff[ks]), as_v8<T>(xf[ks]), hacc[i]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    u32x4 own[N][2];
#pragma unroll
    for (int i = 0; i < N; ++i) finish_h(g.p[i], hacc[i], own[i]);
    const int xs = nst % CS_DEPTH;   // the X slot after the last stage: free (the partner can still be reading stage nst - 1 only)
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const ChainParams& p = g.p[i];
      u32x4 hf[4];
      exchange(xs, own[i], hf);
      const int ksteps = (p.rb + 15) / 16;
#pragma unroll 1
      for (int sl = 0; sl < cs_run<BWD>(g, i); ++sl) {
        refresh();
        raw_barrier();   // B_i chunk sl is in its slot; the partner has parked slice sl - 1
        u32x2 bl[4], bh[4];
        read_f2(slot_a + (uint32_t)((chunk % CS_NSLOT) * CS_FSLOT) + foff2, bl, bh);
        ++chunk;
        f32x16 yacc;
#pragma unroll
        for (int r = 0; r < 16; ++r) yacc[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
          if (ks < ksteps) yacc = mfma32(as_v8<T>(join2(bl[ks], bh[ks])), as_v8<T>(hf[ks]), yacc);
        __builtin_amdgcn_sched_barrier(0);
        epilogue(p, sl, yacc);
      }
      finish_slices(p, cs_run<BWD>(g, i));
    }
  } else {
    // ================================================================== backward data
    u32x4 hf[N][4];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const ChainParams& p = g.p[i];
      if (i > 0) raw_barrier();   // the partner has read the previous exchange: the X ring may be refilled
      f32x16 hacc;
#pragma unroll
      for (int r = 0; r < 16; ++r) hacc[r] = 0.f;
      const int nst = cs_run<BWD>(g, i);
      const int pre = nst < (CS_DEPTH - 1) ? nst : (CS_DEPTH - 1);
      // (the sources are rebuilt per stage: with dh of the earlier siblings live, keeping them would spill the 4-sibling form)
      for (int st = 0; st < pre; ++st) issue_x(p, x_sources(p), st);
#pragma unroll 1
      for (int st = 0; st < nst; ++st) {
        refresh();
        const int newer = (nst - 1 - st) < (CS_DEPTH - 2) ? (nst - 1 - st) : (CS_DEPTH - 2);
        wait_groups<2>(newer);
        raw_barrier();
        if (st + CS_DEPTH - 1 < nst) issue_x(p, x_sources(p), st + CS_DEPTH - 1);
        u32x4 xf[4], ff[4];
        read_x_stage(ring_a + (uint32_t)((st % CS_DEPTH) * CS_STAGE) + xoff, xf);
        read_f1(slot_a + (uint32_t)((chunk % CS_NSLOT) * CS_FSLOT), ff);
        ++chunk;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) hacc = mfma32(as_v8<T>(ff[ks]), as_v8<T>(xf[ks]), hacc);
        __builtin_amdgcn_sched_barrier(0);
      }
      u32x4 own[2];
      finish_h(p, hacc, own);
      exchange(nst % CS_DEPTH, own, hf[i]);
    }
    // phase 2: dX^T slice = sum_i A_i^T-chunk . dh_i^T, one accumulator, stored once with beta = grad_beta
    const ChainParams& px = g.p[0];
#pragma unroll 1
    for (int sl = 0; sl < nsl_b; ++sl) {
      refresh();
      f32x16 yacc;
#pragma unroll
      for (int r = 0; r < 16; ++r) yacc[r] = 0.f;
#pragma unroll
      for (int i = 0; i < N; ++i) {
        raw_barrier();   // A_i chunk sl (i = 0: and the partner has parked slice sl - 1)
        u32x2 bl[4], bh[4];
        read_f2(slot_a + (uint32_t)((chunk % CS_NSLOT) * CS_FSLOT) + foff2, bl, bh);
        ++chunk;
        const int ksteps = (g.p[i].rb + 15) / 16;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
          if (ks < ksteps) yacc = mfma32(as_v8<T>(join2(bl[ks], bh[ks])), as_v8<T>(hf[i][ks]), yacc);
        __builtin_amdgcn_sched_barrier(0);
      }
      epilogue(px, sl, yacc);
    }
    finish_slices(px, nsl_b);
  }
}

template <typename T, bool BWD, bool P16, int N>
__global__ __launch_bounds__(CS_THREADS, 4) void chain2_shared_kernel(const ChainGroup grp) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int total = grp.start[1];
  for (int blk = (int)blockIdx.x; blk < total; blk += (int)gridDim.x) {
    int tt = t;
    asm volatile("" : "+v"(tt));   // keeps per-lane address arithmetic inside the iteration (chain2_kernel)
    chain2_shared_block<T, BWD, P16, N>(grp, blk, smem, tt, tt & 63, w);
  }
}

// =================================================================================================
// ps[i]: the chain2 parameter blocks of the siblings as group_chain_params builds them (forward: X = x, Y = y_i; backward:
// X = dY_i, Y = dX, Hsave = dh_i).  The caller has checked the admitted set: same M, same X (forward) / Y (backward) and
// same d_in; returns SOW_ERR_UNSUPPORTED without launching for anything chain2_shared_supported rejects.
bool chain2_shared_supported(const ChainParams* ps, int n, bool bwd, int dtype) {
  if ((dtype != SOW_BF16 && dtype != SOW_F16) || n < 1 || n > C2_MAXG) return false;
  for (int i = 0; i < n; ++i) {
    const ChainParams& p = ps[i];
    if (!chain2_supported(p, dtype) || p.ntb != 0 || p.pad_dst || p.Hload || p.Hpartial || p.M != ps[0].M) return false;
    if (bwd ? (p.D2 != ps[0].D2 || p.Y != ps[0].Y || p.ldy != ps[0].ldy || !p.Hsave) : (p.D1 != ps[0].D1 || p.X != ps[0].X || p.ldx != ps[0].ldx))
      return false;
    const void* Bp = bwd ? p.F1b : p.F2b;
    const int64_t ldB = bwd ? p.ldf1b : p.ldf2b;
    const void* Ap = bwd ? p.F2b : p.F1b;
    const int64_t ldA = bwd ? p.ldf2b : p.ldf1b;
    if ((reinterpret_cast<uintptr_t>(Bp) & 15) || ldB % 8 || (reinterpret_cast<uintptr_t>(Ap) & 3) || ldA != p.rb) return false;
  }
  return true;
}

int launch_chain2_shared(const ChainParams* ps, int n, bool bwd, int dtype, hipStream_t stream) {
  if (!chain2_shared_supported(ps, n, bwd, dtype)) return SOW_ERR_UNSUPPORTED;
  ChainGroup g{};
  g.n = n;
  bool p16 = !sw_on(SW_NO_PARK16);
  for (int i = 0; i < n; ++i) {
    g.p[i] = ps[i];
    g.p[i].nt_store = sw_on(SW_NO_NT_STORE) ? 0 : 1;
    g.p[i].nt_load = sw_on(SW_NT_LOAD) ? 1 : 0;
    g.p[i].pair_flush = 1;
    p16 = p16 && g.p[i].beta == 0.f && !g.p[i].bias;
  }
  const int64_t total = ceil_div(ps[0].M, CS_BM);
  if (total <= 0) return SOW_OK;
  if (total > 0x7fffffff) return SOW_ERR_SHAPE;
  g.start[0] = 0;
  for (int i = 1; i <= C2_MAXG; ++i) g.start[i] = (int)total;
  const int64_t grid = (sw_on(SW_NO_PERSIST) || total < CS_RESIDENT) ? total : CS_RESIDENT;
#define CS_LAUNCH(T, B, P, N)                                                                                      \
  do {                                                                                                             \
    SOW_SET_MAX_LDS_ONCE(CS_LDS, (chain2_shared_kernel<T, B, P, N>));                                              \
    hipLaunchKernelGGL((chain2_shared_kernel<T, B, P, N>), dim3((unsigned)grid), dim3(CS_THREADS), CS_LDS, stream, g); \
  } while (0)
#define CS_BY_N(T, B, P)              \
  do {                                \
    switch (n) {                      \
      case 1: CS_LAUNCH(T, B, P, 1); break; \
      case 2: CS_LAUNCH(T, B, P, 2); break; \
      case 3: CS_LAUNCH(T, B, P, 3); break; \
      default: CS_LAUNCH(T, B, P, 4); break; \
    }                                 \
  } while (0)
#define CS_BY_P(T, B)                  \
  do {                                 \
    if (p16) CS_BY_N(T, B, true);      \
    else CS_BY_N(T, B, false);         \
  } while (0)
  if (dtype == SOW_F16) {
    if (bwd) CS_BY_P(f16_t, true);
    else CS_BY_P(f16_t, false);
  } else {
    if (bwd) CS_BY_P(bf16_t, true);
    else CS_BY_P(bf16_t, false);
  }
#undef CS_BY_P
#undef CS_BY_N
#undef CS_LAUNCH
  SOW_CHECK_LAUNCH();
  return SOW_OK;
}

}  // namespace sow
