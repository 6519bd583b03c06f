// Loads of rows that start at any 2-byte offset (ragged widths), through a buffer descriptor limited to the bytes a
// workgroup may read: whole aligned 16-byte pieces, shifted into place in registers.  Shared by chain_wide.hip and
// gemm_rag.hip.
#pragma once
#include "common.hpp"

namespace sow {

// 16-byte piece at byte `off` of a ragged workgroup's rows (`lim` bytes): the piece that crosses the limit (the end of the
// tensor, for the last workgroup) is read dword by dword, a 2-byte load for a dword cut in half: nothing past the limit is
// requested, and the bytes past it read as 0
__device__ __forceinline__ u32x4 rag_piece(__amdgpu_buffer_rsrc_t rs, uint32_t off, uint32_t lim) {
  if (off + 16 <= lim) return __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
  u32x4 v;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t o = off + 4 * q;
    v[q] = o + 4 <= lim ? __builtin_amdgcn_raw_buffer_load_b32(rs, o, 0, 0)
                        : (o < lim ? (uint32_t)__builtin_amdgcn_raw_buffer_load_b16(rs, o, 0, 0) : 0u);
  }
  return v;
}

// elements gk .. gk + 7 of row `row` (element e = row * D1 + gk of the workgroup's rows), zero past column D1
__device__ __forceinline__ u32x4 rag_load8(__amdgpu_buffer_rsrc_t rs, uint32_t lim, int row, int D1, int gk) {
  const uint32_t e = (uint32_t)row * (uint32_t)D1 + (uint32_t)gk, off = (e >> 3) << 4;
  const int sh = e & 7, ws = sh >> 1;
  const u32x4 p0 = rag_piece(rs, off, lim);
  const u32x4 p1 = sh ? rag_piece(rs, off + 16, lim) : u32x4{0, 0, 0, 0};
  const uint32_t d[8] = {p0[0], p0[1], p0[2], p0[3], p1[0], p1[1], p1[2], p1[3]};
  uint32_t s5[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) s5[j] = ws == 0 ? d[j] : ws == 1 ? d[j + 1] : ws == 2 ? d[j + 2] : d[j + 3 < 8 ? j + 3 : 7];
  u32x4 v;
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = (sh & 1) ? __builtin_amdgcn_alignbit(s5[j + 1], s5[j], 16) : s5[j];
  const int n = D1 - gk;
  if (n < 8) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = 2 * j >= n ? 0u : (2 * j + 1 >= n ? (v[j] & 0xffffu) : v[j]);
  }
  return v;
}

// A span of 8 * (NP - 1) consecutive elements that starts at element `e` of the descriptor's bytes: the NP aligned pieces
// that hold it (issued by load, kept raw while they are in flight) and the 4 * (NP - 1) dwords shifted into place (get).
// The last piece is not requested when the span starts on a piece boundary.
template <int NP> struct RagSpan {
  u32x4 p[NP];
  int sh;   // elements between the first piece's start and the span's (0 .. 7)

  __device__ __forceinline__ void load(__amdgpu_buffer_rsrc_t rs, uint32_t lim, uint32_t e) {
    const uint32_t off = (e >> 3) << 4;
    sh = e & 7;
#pragma unroll
    for (int i = 0; i < NP - 1; ++i) p[i] = rag_piece(rs, off + 16 * i, lim);
    p[NP - 1] = sh ? rag_piece(rs, off + 16 * (NP - 1), lim) : u32x4{0, 0, 0, 0};
  }
  __device__ __forceinline__ void zero() {
    sh = 0;
#pragma unroll
    for (int i = 0; i < NP; ++i) p[i] = u32x4{0, 0, 0, 0};
  }
  // out[j] = elements 2 j, 2 j + 1 of the span; elements >= n (n >= 0) are zeroed
  __device__ __forceinline__ void get(uint32_t (&out)[4 * (NP - 1)], int n) const {
    constexpr int ND = 4 * (NP - 1);
    // The stages are register vectors, not arrays: a select between two elements of an array becomes a load at a
    // selected address, and the array then lives in scratch memory.
    typedef uint32_t VD __attribute__((ext_vector_type(ND + 4)));
    typedef uint32_t VA __attribute__((ext_vector_type(ND + 2)));
    typedef uint32_t VB __attribute__((ext_vector_type(ND + 1)));
    VD d;
    VA a;
    VB b;
#pragma unroll
    for (int j = 0; j < ND + 4; ++j) d[j] = p[j >> 2][j & 3];
    // dword shift (sh >> 1) in two conditional steps, then the half-dword shift (v_alignbit by 0 or 16 bits)
    const bool s4 = sh & 4, s2 = sh & 2;
    const uint32_t hs = (sh & 1) * 16;
#pragma unroll
    for (int j = 0; j < ND + 2; ++j) a[j] = s4 ? d[j + 2] : d[j];
#pragma unroll
    for (int j = 0; j < ND + 1; ++j) b[j] = s2 ? a[j + 1] : a[j];
#pragma unroll
    for (int j = 0; j < ND; ++j) out[j] = __builtin_amdgcn_alignbit(b[j + 1], b[j], hs);
    if (n < 2 * ND) {
#pragma unroll
      for (int j = 0; j < ND; ++j) out[j] = 2 * j >= n ? 0u : (2 * j + 1 >= n ? (out[j] & 0xffffu) : out[j]);
    }
  }
};

}  // namespace sow
