// Parameter blocks and host launchers shared between the kernel translation units and api.hip.
#pragma once
#include "common.hpp"

namespace sow {
// chain.hip
struct ChainParams {
  const void* X;
  void* Y;
  const void *F1a, *F1b, *F2a, *F2b;
  void* Hsave;
  const void* bias;
  int64_t M, ldx, ldy, ldf1a, ldf1b, ldf2a, ldf2b;
  int D1, D2, ra, rb;
  float scale, beta;
  int fast_factors;
  // side job of the bf16 streaming kernel: out[rows, 64] = [in[rows, r] | 0] (the zero-padded A that the dense
  // backward's K-extension DMAs row by row); workgroup b copies rows 64 b .. 64 b + 63.  nullptr = none.
  const void* pad_src;
  void* pad_dst;
  int pad_rows, pad_r;
  // Short-T split of the streaming kernels (chain2 / chain2f) (grid = ntb token blocks x splits; ntb = 0: no split):
  //   st_per > 0: workgroup (tb, s) runs phase 1 over stages [s*st_per, ..) only and writes its fp32 partial H to
  //               Hpartial[s][M][64] (no phase 2; h_reduce sums, scales, masks and casts into Hsave);
  //   sl_per > 0: workgroup (tb, s) skips phase 1, takes H from Hload [M, 64] and runs phase 2 over slices
  //               [s*sl_per, ..) only.
  int ntb, st_per, sl_per;
  float* Hpartial;
  const void* Hload;
  int nt_store;   // chain2: write Y with the non-temporal hint
  int nt_load;    // chain2 (experiment): stream X with the non-temporal hint
  int h_rows;     // chain2: write Hsave as whole 128-byte rows with the non-temporal hint (through an LDS image)
  int pair_flush; // chain2: store two output slices at a time (256-byte pieces per row)
  int row_align;  // chain2 (set by launch_chain2_group): bit 0 / bit 1 = X stages / Y slices cut on 128-byte lines of every row
  int x_pair;     // chain2 (set by launch_chain2_group): X stages are issued two at a time (256 contiguous bytes per row)
  // chain3f (fp32, T >= 8192): scratch for the pre-split factor planes (chain3f_plane_bytes(D1, D2), 16-byte aligned,
  // from the caller's workspace); nullptr = not available, the launch falls back to chain2f
  void* planes;
  size_t planes_bytes;
};
int launch_chain(ChainParams p, int dtype, bool bwd, hipStream_t stream);
// chain2.hip (bf16 / f16 streaming version; dtype SOW_BF16 or SOW_F16)
constexpr int C2_MAXG = 4;   // layers per grouped launch
struct ChainGroup {
  ChainParams p[C2_MAXG];
  int start[C2_MAXG + 1];    // first workgroup of layer i; start[n..] = grid size
  int n;
  uint64_t* stamps;          // debug builds (SOW_STAMPS): [blocks][8] timeline, else nullptr
};
extern void* g_chain2_stamps;
bool chain2_supported(const ChainParams& p, int dtype);
int launch_chain2(const ChainParams& p, bool bwd, int dtype, hipStream_t stream);
// one grid for n <= C2_MAXG independent layers of the same direction (each one chain2_supported)
int launch_chain2_group(const ChainParams* ps, int n, bool bwd, int dtype, hipStream_t stream);
// chain2_shared.hip: n <= C2_MAXG sibling layers on ONE input in one grid (forward: one X; backward: one summed dX);
// SOW_ERR_UNSUPPORTED (nothing launched) unless chain2_shared_supported
bool chain2_shared_supported(const ChainParams* ps, int n, bool bwd, int dtype);
int launch_chain2_shared(const ChainParams* ps, int n, bool bwd, int dtype, hipStream_t stream);
int launch_h_reduce(const float* Hpartial, int nsplit, void* Hsave, int64_t M, int rb, float scale, int dtype,
                    hipStream_t stream);
// chain2f.hip (fp32 streaming version)
bool chain2f_supported(const ChainParams& p, int dtype);
int launch_chain2f(const ChainParams& p, bool bwd, hipStream_t stream);
// chain3f.hip (fp32 streaming version with pre-split factor planes, 128-token workgroups)
size_t chain3f_plane_bytes(int d_in, int d_out);
bool chain3f_supported(const ChainParams& p, int dtype);
int launch_chain3f(const ChainParams& p, bool bwd, hipStream_t stream);
// skinny_tn.hip
struct TnJob {
  const void* M;
  const void* S;
  float* partial;
  int64_t ldm;
  int D;
  int ones_col;
  int ncg;
  int vec;
  int ones_col_in_s;  // S already carries 1.0 in column `ones_col` (or ones_col < 0): the DMA path cannot patch it
};
struct TnParams {
  TnJob job[2];
  int njobs;
  int64_t T;
  int ns;
  int slab_len;
};
struct ReduceJob {
  const float* partial;
  void* out;
  void* colsum;
  int64_t out_ld;
  int D, Dpad, r;
  int transpose;
  int ones_col;
  float alpha, beta;
  int ns;   // slab count of THIS job (group-planned slabs, tn_rows_plan); 0 = ReduceParams::ns
};
struct ReduceParams {
  ReduceJob job[2];
  int njobs;
  int ns;
  int blocks0;
};
// Every way a layer's weight gradients are computed (the rule: skinny_tn.hip, above tn_shape_kernel).  Per kernel: 64-column
// groups a workgroup owns (tn_groups_per_block) and what the slab length must be a multiple of (tn_slab_mult).
enum TnKernel {
  TN_NONE,        // no blocks: nothing is launched
  TN_GENERIC,     // tn_partial_kernel<T>: 1 group; any operands, any slab length
  TN_DMA,         // tn_partial_dma_kernel<T> (bf16 / f16): 1 group; slab_len % 16
  TN_DMA_WIDE,    // tn_partial_dma_wide_kernel (bf16 / f16; also n layers in one grid, launch_tn_group): 2 groups; slab_len % 16
  TN_ROWS,        // tn_partial_rows_kernel (bf16 / f16, grouped): all groups of a slab, 16 per column range; slab_len % 32, own plan
  TN_F32_X3,      // tn_partial_dma_f32_kernel<true> (3 x bf16): 1 group; slab_len % 8
  TN_F32_EXACT,   // tn_partial_dma_f32_kernel<false> (fp32 MFMAs): 1 group; slab_len % 8
  TN_F32_WIDE,    // tn_partial_dma_f32_wide_kernel: 2 groups; slab_len % 8
  TN_F32_QUAD,    // tn_partial_f32_quad_kernel: 4 groups, grid padded to a multiple of 8 slabs per operand; slab_len % 32
  TN_WIDE_RANK,   // r > 64: tnw_partial_kernel + tnw_reduce_kernel (launch_tn_wide)
  TN_GEMM_PAIR,   // r > 64: two transposed GEMMs and a column sum
};
constexpr int tn_groups_per_block(TnKernel k) { return k == TN_F32_QUAD ? 4 : (k == TN_DMA_WIDE || k == TN_F32_WIDE) ? 2 : 1; }
constexpr int tn_slab_mult(TnKernel k) {
  return (k == TN_ROWS || k == TN_F32_QUAD) ? 32 : (k == TN_DMA || k == TN_DMA_WIDE) ? 16 : (k == TN_F32_X3 || k == TN_F32_EXACT || k == TN_F32_WIDE) ? 8 : 1;
}
// what every LDS-DMA kernel asks of an operand: D and ldm multiples of 16 bytes' worth of elements, M and S 16-byte aligned
// (a TnJob: and the ones column already in S)
bool tn_operand_ok(const void* M, const void* S, int64_t ldm, int D, int elems_per_16B);
bool tn_operand_ok(const TnJob& J, int elems_per_16B);
// the kernel a layer of this shape takes when its operands are aligned: a function of shape, dtype and switches
TnKernel tn_shape_kernel(int64_t T, int d_in, int d_out, int dtype);
TnKernel pick_tn(const TnParams& p, int dtype);      // reads operands and switches, launches nothing
int tn_blocks(TnKernel k, const TnParams& p);        // blocks of work = the grid (the persistent kernels run them on <= 256 workgroups)
int launch_picked_tn(TnKernel k, const TnParams& p, int dtype, hipStream_t stream);
int tn_pick_slabs(int64_t T, int d_in, int d_out, int dtype, int* slab_len);
size_t tn_partial_bytes(int ns, int D);
// skinny_tn_f32q.hip
int launch_tn_f32q(const TnParams& p, hipStream_t stream);
int launch_tn(const TnParams& p, int dtype, hipStream_t stream);   // pick_tn, then launch_picked_tn
constexpr int TN_MAXG = 8;   // layers per grouped launch of the wide bf16 kernel (a decoder block has 7)
struct TnGroup {
  TnParams p[TN_MAXG];
  int start[TN_MAXG + 1];
  int n;
};
// Row-owner weight-gradient kernel (skinny_tn.hip: tn_partial_rows_kernel): one item per (layer, operand); a workgroup
// owns ALL columns of a token slab (up to 1024 per column range), so S (h / dh) is read once per range instead of once
// per 128 columns.  The slab counts are planned over the whole group (work per block equal across items).
struct TnRowsItem {
  const void* M;      // [T, D] bf16, row pitch ldm
  const void* S;      // [T, 64] bf16
  float* partial;     // [ns][ncg * 64][64] fp32
  int64_t ldm, T;
  int D, ncg;         // columns, 64-column groups
  int nr, gpr, cgw;   // column ranges, groups per range, groups per wave (1 or 2)
  int ns, slab_len;
  int start;          // first block of this item in the grid
};
constexpr int TNR_MAXI = 2 * TN_MAXG;
struct TnRowsGroup {
  TnRowsItem it[TNR_MAXI];
  int n, total;
  int nt_load;   // stream M with the non-temporal hint
};
constexpr int TNR_MAX_SLABS = 40;   // workspace capacity per operand (api.hip: plan_ws)
// n items (T[i] tokens x D[i] columns, at most cap[i] slabs): slab counts such that the blocks of the group fill one
// resident round (256 workgroups) with equal work; false = this group does not suit the kernel (too few / too many blocks)
bool tn_rows_plan(const int64_t* T, const int* D, const int* cap, int n, int* ns_out, int* slab_len_out);
int launch_tn_rows(TnRowsItem* items, int n, int dtype, hipStream_t stream);
int launch_tn_group(const TnParams* ps, int n, int dtype, hipStream_t stream);
int launch_tn_reduce(ReduceParams p, int dtype, hipStream_t stream);
int launch_tn_reduce_batch(const ReduceParams* descs, const int* starts, int n, int total_blocks, int dtype, hipStream_t stream);
// chain_wide.hip (bf16 / f16, even r in (64, 256], D1 and D2 multiples of 8; X, Y, bias 16-byte aligned): the fused
// wide-rank chain  H = rn(hscale * X . F1) (to Hsave [M, r] when non-null),  Y = beta * Y + yscale * H . F2 + bias.
// Forward (bwd = 0): F1 = A [D1][r] (ldf1 = r), F2 = B [r][D2] (ldf2 = D2).  Data gradient (bwd = 1): F1 = B [r][D1]
// (ldf1 = D1), F2 = A [D2][r] (ldf2 = r).  `pack` (16-byte aligned, chain_wide_pack_bytes) receives the packed factors.
struct WideArgs {
  const void* X;
  void* Y;
  const void *F1, *F2;
  int64_t ldf1, ldf2;
  void* Hsave;
  const void* bias;
  int64_t M;
  int D1, D2, r;
  float hscale, yscale, beta;
  int bwd;
  void* pack;
  size_t pack_bytes;
};
bool chain_wide_shape_ok(int r, int d1, int d2, int dtype);
// ragged widths (include/sow_amd.h): bf16 / f16, even r in [2, 256], d1 or d2 not a multiple of 8.  The same kernels with
// X / Y rows at any 2-byte offset (X, Y, bias bases still 16-byte aligned).  r <= 64 only without Hsave (the low-rank
// accumulator term of an admitted layer); the weight-gradient kernel takes r > 64 only
bool ragged_shape_ok(int r, int d1, int d2, int dtype);
size_t chain_wide_pack_bytes(int r, int d_in, int d_out);
// SOW_ERR_UNSUPPORTED when the shape, the alignment or the scratch does not suit the kernel (nothing launched)
int launch_chain_wide(const WideArgs& a, int dtype, hipStream_t stream);
// chain_wide_acc.hip (bf16 / f16; SOW_FUSE_ACC): a low-rank accumulator term and the live term of a layer as ONE chain,
//   h = [rn(X . Fa1) | rn(scale * X . Fl1)],  Y = rn(h . [Fa2 ; Fl2] + bias),  Hsave [M, 64] = the live columns of h in the
// r <= 64 contract (zeros above r_live, 1.0 in column 63 when r_live < 64), or nullptr.
// Forward (bwd = 0): Fa1 = Q [D1][r_acc], Fl1 = A [D1][r_live], Fa2 = R [r_acc][D2], Fl2 = B [r_live][D2].  Data gradient
// (bwd = 1): Fa1 = R [r_acc][D1], Fl1 = B [r_live][D1], Fa2 = Q [D2][r_acc], Fl2 = A [D2][r_live].  `pack` (16-byte aligned,
// chain_wide_pack_bytes(r_acc + r_live, D1, D2)) receives the packed factors.
struct WideAccArgs {
  const void* X;
  void* Y;
  const void *Fa1, *Fl1, *Fa2, *Fl2;
  int64_t ldfa1, ldfl1, ldfa2, ldfl2;
  void* Hsave;
  const void* bias;
  int64_t M;
  int D1, D2, r_acc, r_live;
  float scale;
  int bwd;
  void* pack;
  size_t pack_bytes;
};
// even r_live in [2, 64], even r_acc >= 2, r_acc + r_live <= 256, widths multiples of 8, bf16 / f16
bool fused_acc_shape_ok(int r_live, int r_acc, int d_in, int d_out, int dtype);
// SOW_ERR_UNSUPPORTED when the shape, the alignment (X, Y, bias, Hsave, pack: 16 bytes) or the scratch does not suit the
// kernel (nothing launched)
int launch_chain_wide_acc(const WideAccArgs& a, int dtype, hipStream_t stream);
// chain_deep_acc.hip (bf16 / f16; SOW_FUSE_ACC_DEEP): the same chain for 256 < r_acc + r_live <= 960, the H columns computed
// in groups of 256 and kept in dynamic LDS (deep_acc_lds_bytes: 128 bytes per padded column + a 40 KiB stage, at most 160
// KiB).  The operands, the pack and the results' contract are launch_chain_wide_acc's.
// even r_live in [2, 64], even r_acc >= 2, 256 < r_acc + r_live <= 960, widths multiples of 8, bf16 / f16
bool deep_acc_shape_ok(int r_live, int r_acc, int d_in, int d_out, int dtype);
size_t deep_acc_lds_bytes(int r_tot);
// SOW_ERR_UNSUPPORTED when the shape, the alignment (X, Y, bias, Hsave, pack: 16 bytes) or the scratch does not suit the
// kernel (nothing launched)
int launch_chain_deep_acc(const WideAccArgs& a, int dtype, hipStream_t stream);
// chain_shared_acc.hip (bf16 / f16): the data gradients of n <= 4 sibling layers with low-rank accumulators on one input,
// summed on chip:  dh_i as launch_chain_wide_acc(bwd = 1) leaves it,  dX = rn(beta dX + sum_i h_i . [Q_i^T ; A_i^T]).
// sib[i]: the sibling's operands as for launch_chain_wide_acc with bwd = 1 (X = dY_i, Hsave = dh_i, its own pack region; Y
// and bias are not read); one M and one D2 = d_in for the set.  Two launches whatever n.
// The LDS plan of a set, from r_tot[i] = r_acc_i + r_live_i: its bytes (0: n out of range), and whether it fits (160 KiB)
size_t shared_acc_lds_bytes(const int* r_tot, int n);
bool shared_acc_lds_ok(const int* r_tot, int n);
// SOW_ERR_UNSUPPORTED when a shape, the LDS plan, an alignment (dY_i, dh_i, pack, dX: 16 bytes) or the scratch does not suit
// the kernel (nothing launched)
int launch_chain_shared_acc(const WideAccArgs* sib, int n, void* dX, float beta, int dtype, hipStream_t stream);
// skinny_tn_wide.hip: weight gradients of a wide-rank layer, token-slab partials + fixed-order reduction
struct TnwParams {
  const void* M[2];     // x [T, d_in], dY [T, d_out]
  const void* S[2];     // dh [T, r], h [T, r]
  float* partial[2];    // [ns][Dpad][r_pad] fp32
  float* colsum;        // [ns][Dpad of dY] fp32 (dbias), or nullptr
  int D[2], ncg[2];
  int64_t T;
  int r, r_pad, ns, slab_len;
};
struct TnwReduce {
  const float *P0, *P1, *CS;
  void *dA, *dB, *dbias;
  int D0, D1, r, r_pad, ns;
  float scale, beta;
};
bool tnw_shape_ok(int r, int d_in, int d_out, int dtype);
// x, dh, dY, h as launch_tn_wide wants them: 4-byte aligned (ragged widths: x and dY at any 2-byte offset)
bool tnw_operands_ok(const void* x, const void* dh, const void* dy, const void* h, bool rag);
int tnw_pick_slabs(int64_t T, int d_in, int d_out, int* slab_len);
size_t tnw_partial_bytes(int64_t T, int d_in, int d_out, int r);
// dA = x^T dh, dB = scale h^T dY, dbias = colsum(dY), each g = beta g + new; `ws` 256-byte aligned (tnw_partial_bytes);
// the gradients are of out_dtype (dtype, or SOW_F32)
int launch_tn_wide(const void* x, const void* dh, const void* dy, const void* h, void* dA, void* dB, void* dbias, int64_t T,
                   int d_in, int d_out, int r, float scale, float beta, int dtype, int out_dtype, void* ws, size_t ws_bytes,
                   hipStream_t stream);
// skinny_fwd.hip: the fused forward of generation-sized calls (T <= 32, or T <= 64 through the four-row-tile forms of phase A: rows64; bf16 / f16, r <= 64, dense accumulator or none), n <=
// SK_MAXL independent layers in two launches: W streamed once by a grid over (column range) x (K-slab), fp32 slab partials
// through the workspace, summed in slab order with h . B and the bias and rounded once.  An E4M3 accumulator (SOW_ACC_DENSE_FP8:
// W = the codes, 1 byte per element, wexp = the column exponents) is streamed as bytes by instantiations of the same two
// kernels: 128-column ranges, codes converted unscaled in registers, the column's 2^e applied to the slab-order sum in phase B.
// An MXFP4 accumulator (SOW_ACC_DENSE_FP4: W = the packed E2M1 codes [d_in / 2][d_out], wexp = the E8M0 block scales
// [d_in / 32][d_out]) takes the same geometry with the scale applied in the conversion, and the plain second kernel.
// The dense layers of one call are all of one kind.
// A dense accumulator stored as codes, with scales in acc_up's place; and a kind value of include/sow_amd.h (a format is added to both)
constexpr bool acc_is_codes(int kind) { return kind == SOW_ACC_DENSE_FP8 || kind == SOW_ACC_DENSE_FP4; }
constexpr bool acc_kind_known(int kind) { return kind == SOW_ACC_NONE || kind == SOW_ACC_LOWRANK || kind == SOW_ACC_DENSE || acc_is_codes(kind); }
constexpr int SK_MAXL = 16;
struct SkLayer {
  const void *x, *W, *A, *B, *bias;   // W = the dense accumulator [d_in][d_out], its codes (E4M3 [d_in][d_out], MXFP4 [d_in / 2][d_out]), or nullptr
                                      // A, B, bias: of the compute dtype, or all fp32 (launch_skinny_fwd's param_f32)
  void* y;
  float *Py, *Ph;                     // slab partials [S][T][d_out] (nullptr without W) and [S][T][64]
  int T, d_in, d_out, r;
  int S, KS, ncr, startA, startB;     // filled in by launch_skinny_fwd (skinny_plan)
  float scale;
  const int8_t* wexp;                 // the scales of codes in W (E4M3: int8 column exponents [d_out]; MXFP4: E8M0 bytes [d_in / 32][d_out]), or nullptr
  void* hout;                         // short-row forms: where phase B stores h / dh, [T][64], or nullptr (a slot of its own: the code forms need both)
};
// K-slabs, slab length and phase-A column ranges of a layer: a pure function of the shape
void skinny_plan(int d_in, int d_out, int acc_kind, int* S, int* KS, int* ncr);
// ... of sow_forward_skinny_rows: skinny_plan for T <= 32, a plan of fewer, longer slabs (by T) for 33 <= T <= 64
void skinny_rows_plan(int64_t T, int d_in, int d_out, int acc_kind, int* S, int* KS, int* ncr);
size_t skinny_py_bytes(int64_t T, int d_out, int S);
size_t skinny_ph_bytes(int64_t T, int S);
// acc_kind: the kind of the call's dense layers (SOW_ACC_DENSE, SOW_ACC_DENSE_FP8 or SOW_ACC_DENSE_FP4; any of them without one)
// param_f32: A, B and bias are fp32 (16-byte aligned as before), rounded once to `dtype` in registers by both kernels
// rows64: every layer has 33 <= T <= 64 and takes skinny_rows_plan and the four-row-tile phase A (sow_forward_skinny_rows);
// otherwise every layer has T <= 32
int launch_skinny_fwd(const SkLayer* layers, int n, int dtype, int acc_kind, bool param_f32, hipStream_t stream, bool rows64 = false);
// Short batches (sow_forward_short / sow_backward_short: SOW_ACC_DENSE, 1 <= T <= SK_SHORT_MAX): a layer is cut into row blocks
// of 64, every block one SkLayer entry on the same W.  short_rows_plan: the slab plan ALL blocks of a layer take, counted over
// blocks x column ranges x slabs; K = the contraction width, N = the output width (forward: d_in, d_out; data gradient: d_out,
// d_in), kq = the k per round of the four waves (SK_SHORT_KQ_FWD / _BWD).  A pure function of its arguments.
constexpr int SK_SHORT_MAX = 1024, SK_SHORT_KQ_FWD = 128, SK_SHORT_KQ_BWD = 256;
void short_rows_plan(int64_t T, int K, int N, int kq, int* S, int* KS, int* ncr);
// entries: any number of row blocks (1 <= T <= 64 each) with S, KS and ncr set from short_rows_plan, Py / Ph per block, hout = h_save
// / dh of the block or nullptr; launched 16 at a time, one launch pair each.  bwd: the entries carry the data gradient's
// operands in the forward's fields -- x = dY, W = W_acc (read transposed in place), A = B [r][d_out], B = A [d_in][r], y = dX,
// d_in = the layer's d_out (contraction), d_out = the layer's d_in (output), no bias
// acc_kind: SOW_ACC_DENSE, or the code kind of ALL entries (sow_forward_short_codes / sow_backward_short_codes: W = the codes, wexp = the
// scales).  On codes the forward's phase A is the RT = 4 code form (128-column ranges: short_codes_plan), the data gradient keeps
// the plain geometry (short_rows_plan) and dequantises W in registers
int launch_skinny_short(const SkLayer* entries, int n, int dtype, bool bwd, hipStream_t stream, int acc_kind = SOW_ACC_DENSE);
// the forward's slab plan on codes, next to short_rows_plan: the row blocks counted with 128-column ranges, slabs of whole MX
// blocks and whole rounds (SK_SHORT_KQ_FWD), at most 512.  A pure function of its arguments.
void short_codes_plan(int64_t T, int K, int N, int* S, int* KS, int* ncr);
// gemm.hip
int launch_gemm(const void* A, int64_t lda, bool transA, const void* B, int64_t ldb, bool transB, void* C, int64_t ldc,
                const void* bias, int64_t M, int N, int K, float alpha, float beta, int dtype, hipStream_t stream);
// the same with C (and bias) of c_dtype: c_dtype = dtype, or SOW_F32 for bf16 / f16 operands (fp32 weight gradients)
int launch_gemm_out(const void* A, int64_t lda, bool transA, const void* B, int64_t ldb, bool transB, void* C, int64_t ldc,
                    const void* bias, int64_t M, int N, int K, float alpha, float beta, int dtype, int c_dtype,
                    hipStream_t stream);
// gemm_rag.hip: C[M, N] = A[M, K] . op(B) (alpha = 1, beta = 0, no bias) for bf16 / f16 operands whose leading dimensions are
// any element counts (rows at any 2-byte offset; A, B, C bases 16-byte aligned).  transB: B stored [N, K].  B is read in
// place: no copy, no workspace.  SOW_ERR_UNSUPPORTED (nothing launched) unless gemm_rag_supported
bool gemm_rag_supported(const void* A, int64_t lda, const void* B, int64_t ldb, bool transB, const void* C, int64_t ldc, int64_t M,
                        int N, int K, int dtype);
int launch_gemm_rag(const void* A, int64_t lda, const void* B, int64_t ldb, bool transB, void* C, int64_t ldc, int64_t M, int N,
                    int K, int dtype, hipStream_t stream);
// gemm_x3.hip: the same contract for fp32 tensors on the bf16 matrix pipe (3 x bf16 splits); vector-aligned operands only
int launch_gemm_x3(const void* A, int64_t lda, bool transA, const void* B, int64_t ldb, bool transB, void* C, int64_t ldc,
                   const void* bias, int64_t M, int N, int K, float alpha, float beta, hipStream_t stream);
// The streaming GEMM family with an optional K-extension (gemm2 / gemm3 / gemm3s / gemm4):
//     C[M,N] = alpha * (A[M,K] . op(B) + A2[M,64] . op(B2)) + beta * C + bias[N]
// nt: op(B) = B^T, B given as [N, K] (B2 as [N, 64]); else B is [K, N] (B2 [k2, N]).  A2 = nullptr: no extension.
// Which kernel runs a product is decided in api.hip (pick_gemm); the launchers below launch their own kernel only.
struct ExtGemm {
  const void *A, *B, *A2, *B2;
  void* C;
  const void* bias;
  int64_t M, lda, ldb, lda2, ldb2, ldc;
  int N, K, k2;
  bool nt;
  float alpha, beta;
};
// what every kernel of the family asks of the operands: A, B, C given; K, N, lda, ldb, ldc multiples of 8; A, B, C, bias
// 16-byte aligned; with an extension B2 given, lda2 and ldb2 multiples of 8, A2 and B2 16-byte aligned
bool ext_gemm_operands_ok(const ExtGemm& g);
// the kernel-argument block of gemm2_kernel / gemm3_kernel / gemm3s_kernel (bf16)
struct ExtGemmParams {
  const bf16_t* A;
  const bf16_t* B;
  const bf16_t* A2;   // [M, 64] or nullptr
  const bf16_t* B2;   // NT: [N, 64]; NN: [k2, N]
  bf16_t* C;
  const bf16_t* bias;
  int64_t M, lda, ldb, lda2, ldb2, ldc;
  int N, K, k2;
  float alpha, beta;
};
ExtGemmParams ext_gemm_params(const ExtGemm& g);   // k2 clamped to the 64 rows of the extension
// gemm2.hip (bf16; 256x256 tiles, 8 waves, 32-wide K stages)
int launch_gemm2(const ExtGemm& g, hipStream_t stream);
int launch_pad64(const void* in, void* out, int rows, int r, hipStream_t stream);
// gemm3.hip (bf16; one wave per SIMD, 128x128 per wave, hand-interleaved k-loop: long K)
int launch_gemm3(const ExtGemm& g, hipStream_t stream);
// gemm3s.hip (bf16; 128x128 tiles for products with few 256x256 tiles: short M)
int launch_gemm3s(const ExtGemm& g, hipStream_t stream);
// gemm4.hip (256x256x64 tiles, two wave groups in anti-phase, v_mfma_f32_16x16x32_bf16 / _f16).  dtype: SOW_BF16 or SOW_F16
// (gemm4_f16_kernel).  ext_gemm_operands_ok and M >= 1, N >= 64, K >= 64
bool gemm4_supported(const ExtGemm& g, int dtype);
// ws / ws_bytes: optional scratch for split-K (gemm4_splitk_bytes; short M), nullptr = never split
int launch_gemm4(const ExtGemm& g, int dtype, void* ws, size_t ws_bytes, hipStream_t stream);
// split-K of gemm4 for short M (<= 128 output tiles): scratch bytes (0 = the shape does not split), and the split count a
// launch with this scratch takes (1 = none)
size_t gemm4_splitk_bytes(int64_t M, int N, int K, bool has_ext);
int gemm4_splits(int64_t M, int N, int K, bool has_ext, const void* ws, size_t ws_bytes);
// The same product with the projection H = hscale * X . op(F) computed by the kernel and used as the extension's A operand
// (one launch per pass):  C = X . op(W) + H . op(G) + bias, H [M, 64] saved.  The operands of one layer; nt is a separate
// argument because a grouped launch has one for the whole group.
struct ProjGemm {
  const void *X, *W, *F, *G;
  void* C;
  const void* bias;
  void* H;
  int64_t M, ldx, ldw, ldf, ldg, ldc;
  int N, K, r;
  float hscale;
};
// gemm4.hip, gemm4h form: a streaming pass over the row panel ahead of the main loop; F / G zero-padded to 64 columns where
// they are k-major
bool gemm4h_supported(const ProjGemm& g, bool nt, int dtype);
int launch_gemm4h(const ProjGemm& g, bool nt, int dtype, hipStream_t stream);
// gemm2h.hip (bf16): n <= 4 layers in one launch, every one gemm2h_supported
bool gemm2h_supported(const ProjGemm& g, bool nt, int dtype);
int launch_gemm2h_group(const ProjGemm* g, int n, bool nt, hipStream_t stream);
// qr.hip
int launch_cast_copy(const void* src, int64_t lds, int src_dtype, void* dst, int64_t ldd, int dst_dtype, int64_t rows,
                     int cols, hipStream_t stream);
// dst[k][n] = e4m3(q[k][n]) * 2^exps[n] in bf16 / f16 (exact): the image of an E4M3 accumulator; d_out % 8 == 0, ldd % 8 == 0,
// q 8-byte and dst 16-byte aligned
int launch_acc_dequantize(const void* q, const void* exps, int d_in, int d_out, void* dst, int64_t ldd, int dst_dtype,
                          hipStream_t stream);
// dst[k][n] = e2m1(code(k, n)) * 2^(scales[k / 32][n] - 127) in bf16 / f16 (exact): the image of an MXFP4 accumulator; d_in % 32
// == 0, d_out % 8 == 0, ldd % 8 == 0, q and scales 8-byte and dst 16-byte aligned
int launch_acc_dequantize_fp4(const void* q, const void* scales, int d_in, int d_out, void* dst, int64_t ldd, int dst_dtype,
                              hipStream_t stream);
int launch_qr_panel(const void* W, int64_t ldw, int in_dtype, int m, int kc, int r, float* Pt, float* Qt,
                    hipStream_t stream);
int launch_qr_copy_out(const float* Qt, const float* Pt, void* Q, int64_t ldq, void* R, int64_t ldr, int out_dtype, int m,
                       int kc, int r, int k_rows, hipStream_t stream);
// qr_blocked.hip: the same factorisation by blocks of 32 columns (compact WY), trailing updates and Q on the whole chip.
// T: qr_blocked_t_floats(kc) floats of workspace, written before they are read.  Same Pt / Qt contents on return as
// launch_qr_panel (R on and above the diagonal of Pt, Q[:, :r] in Qt), up to rounding; SOW_ERR_UNSUPPORTED (nothing
// launched) for m > 38400 rows, where the block's reflector no longer fits the LDS -- launch_qr_panel's limit as well.
size_t qr_blocked_t_floats(int kc);
int launch_qr_blocked(const void* W, int64_t ldw, int in_dtype, int m, int kc, int r, float* Pt, float* Qt, float* T,
                      hipStream_t stream);
// accumulate.hip: batched Householder panels (one 1024-thread workgroup per matrix; Pt [kc][m] column-major panel in,
// factored in place; Qt [r_new][m] = Q[:, :r_new] out)
struct QrItem {
  float* Pt;
  float* Qt;
  int m, kc, r_new, pad;
};
int launch_qr_panel_batch(const QrItem* items, int n, hipStream_t stream);
// accumulate.hip: the periodic step of many layers, one launch per phase
struct AccItem {
  void* acc;            // [d_in, d_out] dense accumulator, acc = beta * acc + scale * A . B
  const void* A;        // [d_in, r]
  const void* B;        // [r, d_out]
  const void* draw;     // [d_in, >= kc] Gaussian draw (row stride ld_draw) or nullptr: no re-initialisation
  void* A_new;          // [d_in, r_new] <- Q[:, :r_new] of the draw (may alias A)
  float* Pt;            // workspace: kc * d_in floats
  float* Qt;            // workspace: r_new * d_in floats
  int64_t ld_draw;
  int d_in, d_out, r, r_new, kc;
  float scale, beta;
};
constexpr int ACC_MAXB = 40;   // layers per launch: the by-value argument block is 40 x 96 bytes + 8 = 3848 bytes, under HIP's 4-KiB limit
struct AccBatch {
  AccItem it[ACC_MAXB];
  int n;
};
static_assert(sizeof(AccBatch) <= 4096, "by-value kernel arguments must stay under 4 KiB");
int launch_accumulate_batch(const AccItem* items, int n, int dtype, hipStream_t stream);
// misc.hip
int launch_multi_zero(void* const* ptrs, const int64_t* bytes, int n, hipStream_t stream);
int launch_adamw_flat(void* p, const void* g, void* m, void* v, int64_t n, float lr, double b1, double b2, float eps,
                      float wd, int step, float grad_scale, int dtype, int state_dtype, hipStream_t stream);
int launch_adamw_flat_seg(void* p, const void* g, void* m, void* v, const sow_adamw_segment* segs, int n_segs, double b1,
                          double b2, float eps, float grad_scale, int dtype, int state_dtype, hipStream_t stream);
int launch_adamw_flat_seg_stats(void* p, const void* g, void* m, void* v, const sow_adamw_segment* segs, const int* seg_counter,
                                int n_segs, double b1, double b2, float eps, const sow_grad_stats* stats, int skip_nonfinite,
                                const int32_t* skip_counters, int n_counters, int dtype, int state_dtype, hipStream_t stream);
// grad_stats.hip
size_t grad_stats_workspace_bytes(int64_t n);
int launch_grad_stats(const void* grad, int64_t n, int dtype, float grad_scale, float max_norm, const double* extra_sumsq,
                      const float* loss_scale, const float* extra_found_inf, int32_t* skip_counters, int n_counters,
                      void* workspace, size_t workspace_bytes, sow_grad_stats* out, hipStream_t stream);
int launch_ttadam_dense(float* p, const float* g, float* m, float* v, int64_t n, double b1, double b2, float eps,
                        float step_size, float lr_wd, int clamp_v, hipStream_t stream);
int launch_tt_kron_core(const float* A, const float* B, float* out, int ra0, int rb0, int ij, int ra1, int rb1,
                        hipStream_t stream);
int launch_absmax(const float* x, int64_t n, float* out, hipStream_t stream);
int launch_small_inverse(const float* A, float* out, int batch, int r, hipStream_t stream);
int launch_axpby(const void* x, void* y, int64_t n, float a, float b, int dtype, hipStream_t stream);
// misc.hip: fp32 parameter operands (SOW_PARAM_F32) rounded once, RNE, to the compute dtype (bf16 / f16), many tensors per
// launch; dst 16-byte aligned (the pack region of a layer's workspace)
struct PackItem {
  const float* src;
  void* dst;
  int64_t n;   // elements
};
int launch_pack_params(const PackItem* items, int n, int dtype, hipStream_t stream);
}  // namespace sow
