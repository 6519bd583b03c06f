// Tile code shared by the fused wide chains (chain_wide.hip, chain_wide_acc.hip): one 64-token workgroup of 256 threads,
// 64 KiB of LDS split into `big` (32 KiB: the F1 image [r_pad][64] of phase 1, then H as r_pad / 64 panels [64][64]) and
// `small` (32 KiB: the X image [64][64] of phase 1, then the F2 panels [64][64] of phase 2, reused as the epilogue scratch).
//   cw_phase1: acc = X . F1 over K = D1 in 64-wide steps; the H tiles (2 token halves x r_pad / 32 column tiles) are dealt
//              round-robin to the waves: wave w owns tiles w, w + 4, ... (<= 4 each); tile j = token half j & 1, columns
//              32 (j >> 1) ..; ends with a barrier (every wave done with the F1 / X images)
//   (the caller rounds acc into the H panels at cw_panel_off, synchronises, saves what it saves)
//   cw_phase2: Y = beta * Y + yscale * H . F2 + bias, 64 output columns at a time, wave (wm, wn) owns a 32 x 32 tile
// The factors come packed: F1T [r_pad][ldf1t] (row c = column c of H), F2T [D2][r_pad] (row n = output column n).
// chain_shared_acc.hip runs the same phase 1 once per sibling (cw_phase1_at) into panels of several chains side by side and
// one phase 2 over all of them (cw_phase2_panels), in dynamic LDS of its own plan; chain_deep_acc.hip does the same with the
// column groups of ONE chain.
#pragma once
#include "kernels.hpp"
#include "epilogue.hpp"
#include "rag_load.hpp"

namespace sow {

constexpr int CW_LDS = 65536, CW_PANEL = 64 * 64 * 2;

// byte offset of H[row][k] in the phase-2 image
template <typename T> __device__ __forceinline__ int cw_panel_off(int row, int k) {
  return (k >> 6) * CW_PANEL + bf16_img_off<64>(row, (k & 63) >> 3) + (k & 7) * 2;
}

// RAG: D1 not a multiple of 8 -- a token row of X starts at any 2-byte offset (rag_load.hpp; X itself 16-byte aligned)
// cw_phase1_at: the same for a caller that hands in its thread index (a kernel that runs phase 1 in a loop keeps the per-lane
// address arithmetic inside the iteration that way: chain_shared_acc.hip)
template <typename T, bool RAG>
__device__ __forceinline__ void cw_phase1_at(f32x16 (&acc)[4], char* big, char* small, const T* X, const T* F1T, int64_t M,
                                             int64_t t0, int D1, int ldf1t, int r_pad, const int t) {
  using V8 = typename DT<T>::v8;
  const int lane = t & 63, w = t >> 6, li = lane & 31, lh = lane >> 5;
  const int ntiles = 2 * (r_pad / 32);
  // RAG: the workgroup's token rows as one buffer (base 16-byte aligned: X is, and t0 * D1 * 2 is a multiple of 128)
  const int rows = M - t0 < 64 ? (int)(M - t0) : 64;
  const uint32_t lim = (uint32_t)rows * (uint32_t)D1 * 2u;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(X + t0 * D1), (short)0, (int)lim, 0x00020000);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
  u32x4 xv[2], fv[8];
  auto load1 = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = t + 256 * i, row = idx >> 3, c = idx & 7;
      const int64_t gt = t0 + row;
      const int gk = k0 + c * 8;
      if constexpr (RAG)
        xv[i] = (row < rows && gk < D1) ? rag_load8(rs, lim, row, D1, gk) : u32x4{0, 0, 0, 0};
      else
        xv[i] = (gt < M && gk < D1) ? *(const u32x4*)(X + gt * D1 + gk) : u32x4{0, 0, 0, 0};
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int idx = t + 256 * i, row = idx >> 3, c = idx & 7;
      const int gk = k0 + c * 8;
      fv[i] = (row < r_pad && gk < D1) ? *(const u32x4*)(F1T + (int64_t)row * ldf1t + gk) : u32x4{0, 0, 0, 0};
    }
  };
  auto store1 = [&]() {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = t + 256 * i;
      *(u32x4*)(small + bf16_img_off<64>(idx >> 3, idx & 7)) = xv[i];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int idx = t + 256 * i;
      if ((idx >> 3) < r_pad) *(u32x4*)(big + bf16_img_off<64>(idx >> 3, idx & 7)) = fv[i];
    }
  };
  const int nk = (D1 + 63) / 64;
  load1(0);
  for (int kt = 0; kt < nk; ++kt) {
    __syncthreads();
    store1();
    __syncthreads();
    if (kt + 1 < nk) load1((kt + 1) * 64);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const V8 a0 = *(const V8*)(small + bf16_img_off<64>(li, 2 * ks + lh));
      const V8 a1 = *(const V8*)(small + bf16_img_off<64>(32 + li, 2 * ks + lh));
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = w + 4 * i;
        if (j < ntiles) {
          const V8 b = *(const V8*)(big + bf16_img_off<64>((j >> 1) * 32 + li, 2 * ks + lh));
          acc[i] = mfma32((j & 1) ? a1 : a0, b, acc[i]);
        }
      }
    }
  }
  __syncthreads();   // every wave is done with the F1 / X images
}
template <typename T, bool RAG>
__device__ __forceinline__ void cw_phase1(f32x16 (&acc)[4], char* big, char* small, const T* X, const T* F1T, int64_t M, int64_t t0,
                                          int D1, int ldf1t, int r_pad) {
  cw_phase1_at<T, RAG>(acc, big, small, X, F1T, M, t0, D1, ldf1t, r_pad, threadIdx.x);
}

// VEC: D2 a multiple of 8 (16-byte row pieces of Y), else element by element
template <typename T, bool VEC>
__device__ __forceinline__ void cw_phase2(char* big, char* small, const T* F2T, T* Y, const T* bias, int64_t M, int64_t t0, int D2,
                                          int r_pad, float yscale, float beta, bool nt) {
  using V8 = typename DT<T>::v8;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, li = lane & 31, lh = lane >> 5;
  const int np = r_pad / 64, wm = w >> 1, wn = w & 1;
  u32x4 gv[8];
  auto load2 = [&](int n0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int idx = t + 256 * i, pn = idx >> 9, row = (idx >> 3) & 63, c = idx & 7;
      const int gn = n0 + row;
      gv[i] = (pn < np && gn < D2) ? *(const u32x4*)(F2T + (int64_t)gn * r_pad + pn * 64 + c * 8) : u32x4{0, 0, 0, 0};
    }
  };
  const int nn = (D2 + 63) / 64;
  float* scratch = (float*)small + w * EpiScratch<1>::FLOATS;
  load2(0);
  for (int nb = 0; nb < nn; ++nb) {
    __syncthreads();   // the previous tile's epilogue is done with the scratch
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int idx = t + 256 * i, pn = idx >> 9;
      if (pn < np) *(u32x4*)(small + pn * CW_PANEL + bf16_img_off<64>((idx >> 3) & 63, idx & 7)) = gv[i];
    }
    __syncthreads();
    if (nb + 1 < nn) load2((nb + 1) * 64);
    f32x16 o;
#pragma unroll
    for (int e = 0; e < 16; ++e) o[e] = 0.f;
    for (int pn = 0; pn < np; ++pn) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const V8 a = *(const V8*)(big + pn * CW_PANEL + bf16_img_off<64>(wm * 32 + li, 2 * ks + lh));
        const V8 b = *(const V8*)(small + pn * CW_PANEL + bf16_img_off<64>(wn * 32 + li, 2 * ks + lh));
        o = mfma32(a, b, o);
      }
    }
    __syncthreads();   // the F2 panels are consumed: their space becomes the epilogue scratch
    wave_store_tiles<T, 1, VEC>(&o, scratch, Y, D2, t0 + wm * 32, nb * 64 + wn * 32, M, D2, yscale, beta, bias, lane, nt);
  }
}

// The panels of several chains side by side (chain_shared_acc.hip): H [64 tokens][64 np] as np panels [64][64] at `hp`, summed
// into ONE output.  Panel q multiplies the 64 columns of F2 that start at f2[q] (row n = output column n, row pitch ld[q]
// elements): a sibling's own F2T, 64 pn columns in.  The F2 panels pass through `stage` g at a time (g <= 4; g panels and the
// epilogue scratch fit into `stage`); the fp32 accumulation runs over the panels in ascending q, ascending k inside a panel.
// bias [D2] (or null) is added in fp32 before the one rounding.
// CW_MAXP: four chains of r_pad = 256 -- more than any LDS plan holds (chain_shared_acc.hip admits at most 15 panels), so that
// the table cannot overflow whatever the plan's limit becomes; the launcher checks the count all the same.
constexpr int CW_MAXP = 16;
struct CwPanels {
  const void* f2[CW_MAXP];
  int ld[CW_MAXP];
  int np;
};
// PP: a pointer to CwPanels in any address space (the kernel-argument segment: the entries are then scalar loads at a uniform
// index)
template <typename T, typename PP>
__device__ __forceinline__ void cw_phase2_panels(const char* hp, char* stage, int g, PP P, T* Y, int64_t M, int64_t t0, int D2,
                                                 float beta, bool nt, const int t, const T* bias) {
  using V8 = typename DT<T>::v8;
  const int lane = t & 63, w = t >> 6, li = lane & 31, lh = lane >> 5;
  const int np = P->np, wm = w >> 1, wn = w & 1;
  u32x4 gv[8];
  // thread t stages chunk t & 7 of rows (t >> 3) & 63 + 32 (i & 1) of the group's panel i >> 1
  auto load2 = [&](int n0, int q0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int q = q0 + (i >> 1), row = ((t + 256 * i) >> 3) & 63, gn = n0 + row;
      gv[i] = u32x4{0, 0, 0, 0};
      if ((i >> 1) < g && q < np && gn < D2) gv[i] = *(const u32x4*)((const T*)P->f2[q] + (int64_t)gn * P->ld[q] + (t & 7) * 8);
    }
  };
  const int nn = (D2 + 63) / 64, ngrp = (np + g - 1) / g;
  float* scratch = (float*)stage + w * EpiScratch<1>::FLOATS;
  load2(0, 0);
  for (int nb = 0; nb < nn; ++nb) {
    f32x16 o;
#pragma unroll
    for (int e = 0; e < 16; ++e) o[e] = 0.f;
    for (int grp = 0; grp < ngrp; ++grp) {
      const int q0 = grp * g;
      __syncthreads();   // the previous group's products / the previous tile's epilogue are done with the stage
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if ((i >> 1) < g && q0 + (i >> 1) < np)
          *(u32x4*)(stage + (i >> 1) * CW_PANEL + bf16_img_off<64>(((t + 256 * i) >> 3) & 63, t & 7)) = gv[i];
      __syncthreads();
      if (grp + 1 < ngrp) load2(nb * 64, q0 + g);
      else if (nb + 1 < nn) load2((nb + 1) * 64, 0);
      for (int j = 0; j < g && q0 + j < np; ++j) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const V8 a = *(const V8*)(hp + (q0 + j) * CW_PANEL + bf16_img_off<64>(wm * 32 + li, 2 * ks + lh));
          const V8 b = *(const V8*)(stage + j * CW_PANEL + bf16_img_off<64>(wn * 32 + li, 2 * ks + lh));
          o = mfma32(a, b, o);
        }
      }
    }
    __syncthreads();   // the F2 panels are consumed: their space becomes the epilogue scratch
    wave_store_tiles<T, 1, true>(&o, scratch, Y, D2, t0 + wm * 32, nb * 64 + wn * 32, M, D2, 1.f, beta, bias, lane, nt);
  }
}

// ---- the factor pack of the fused low-rank-accumulator chains (chain_wide_acc.hip, chain_shared_acc.hip) -----------
struct WideAccPack {
  const void *Fa, *Fl;   // accumulator and live source of this image
  int64_t lda, ldl;
  int trans;             // source element (rank k, width index j) = trans ? F[j][k] : F[k][j]
};
struct WideAccPackParams {
  WideAccPack img[2];    // 0: F1T [r_pad][d1p], 1: F2T [D2][r_pad]
  void *f1t, *f2t;
  int r_acc, r_tot, r_pad, D1, d1p, D2;
  int64_t n0, n;         // elements of image 0, of both
};
// element i < p.n of the two images
template <typename T> __device__ __forceinline__ void wide_acc_pack_elem(const WideAccPackParams& p, int64_t i) {
  const int which = i >= p.n0 ? 1 : 0;
  int k, j, D;   // rank index, width index, valid width
  T* dst;
  if (!which) {
    k = (int)(i / p.d1p), j = (int)(i % p.d1p), D = p.D1, dst = (T*)p.f1t + i;
  } else {
    i -= p.n0;
    j = (int)(i / p.r_pad), k = (int)(i % p.r_pad), D = p.D2, dst = (T*)p.f2t + i;
  }
  const WideAccPack& J = p.img[which];
  T v = from_f32<T>(0.f);
  if (k < p.r_tot && j < D) {
    const bool live = k >= p.r_acc;
    const T* src = (const T*)(live ? J.Fl : J.Fa);
    const int64_t ld = live ? J.ldl : J.lda;
    const int kk = live ? k - p.r_acc : k;
    v = J.trans ? src[(int64_t)j * ld + kk] : src[(int64_t)kk * ld + j];
  }
  *dst = v;
}
// one launch packs both images of a layer and direction (chain_wide_acc.hip, chain_deep_acc.hip)
template <typename T> __global__ __launch_bounds__(256) void wide_acc_pack_kernel(const WideAccPackParams p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < p.n) wide_acc_pack_elem<T>(p, i);
}
// The pack of one layer and direction into `a.pack`: F1T at its start, F2T at the next 256-byte boundary.
// forward: F1 = [Q | A] stored [D1][r] (transposed on the way in), F2 = [R ; B] stored [r][D2];
// data gradient: F1 = [R^T | B^T], R / B stored [r][D1] (as stored), F2 = [Q^T ; A^T], Q / A stored [D2][r]
inline WideAccPackParams wide_acc_pack_params(const WideAccArgs& a) {
  const int r_tot = a.r_acc + a.r_live, r_pad = (r_tot + 63) / 64 * 64;
  char* f1t = (char*)a.pack;
  WideAccPackParams pk{};
  pk.img[0] = WideAccPack{a.Fa1, a.Fl1, a.ldfa1, a.ldfl1, a.bwd ? 0 : 1};
  pk.img[1] = WideAccPack{a.Fa2, a.Fl2, a.ldfa2, a.ldfl2, a.bwd ? 1 : 0};
  pk.f1t = f1t, pk.f2t = f1t + (((size_t)r_pad * a.D1 * 2 + 255) & ~(size_t)255);
  pk.r_acc = a.r_acc, pk.r_tot = r_tot, pk.r_pad = r_pad, pk.D1 = a.D1, pk.d1p = a.D1, pk.D2 = a.D2;
  pk.n0 = (int64_t)r_pad * a.D1;
  pk.n = pk.n0 + (int64_t)a.D2 * r_pad;
  return pk;
}

}  // namespace sow
