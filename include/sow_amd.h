/* sow_amd.h -- C ABI of libsow_amd.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for the SoW (Sum-of-Weights) low-rank linear hot path of
 * antoine311200/sow.  The reference has NO foreign-function interface: its hot
 * path is Python (tn_gradient/layer/sow.py, tn_gradient/utils.py,
 * tn_gradient/prepare.py, tn_gradient/tt.py) calling ATen.  Each entry point
 * below replaces the ATen call sequence of the cited reference lines; the
 * host-side mirror (the sow_amd Python package) binds them with ctypes and keeps the
 * reference's class/function surface.
 *
 * Conventions:
 *   - every function returns int: 0 ok, <0 argument error (SOW_ERR_*), >0 hipError_t;
 *   - nothing here allocates or frees device memory or synchronises the device; no mutable global state except
 *     the kernel-selection switches (sow_set_switch), which production code leaves alone;
 *     the caller passes a workspace sized by the matching *_workspace_bytes query;
 *   - all tensors are dense row-major device buffers, 16-byte aligned for the
 *     fast paths (unaligned / odd shapes take slower element-wise paths);
 *   - dtype: SOW_DTYPE_F32 (fp32 tensors; products on the bf16 matrix pipe as 3 x bf16 splits by default, the exact
 *     f32 MFMA under the F32_EXACT switch), SOW_DTYPE_BF16 (bf16 MFMA, f32 accumulate) or SOW_DTYPE_F16 (f16 MFMA, f32
 *     accumulate); the tensor-train entry points (sow_tt_*, sow_ttadam_dense) are fp32 only;
 *   - f16 numerics: every product accumulates in fp32 and each output element is rounded once, to nearest even, to f16;
 *     a result beyond +-65504 becomes +-inf (IEEE rounding, as torch's f16 matmul; no saturation); subnormal outputs are
 *     kept, not flushed; h_save has the bf16 layout (scale * x . A, 64 columns, column 63 = 1.0 when free);
 *   - exact arithmetic: products are exact and every sum is accumulated in fp32, so where the terms of every sum are
 *     multiples of one unit and sum |terms| stays below 2^24 units (and what is stored on the way -- h_save, the internal
 *     dh, the first product of a two-pass accumulator path -- is representable), each output is the correctly rounded exact
 *     result whatever the slab, K-split or sibling order.  SOW_DTYPE_F32 on the 3 x bf16 split: the same holds when one
 *     factor of every product has at most 8 significant bits (the six plane products kept are then the whole product);
 *   - powers of two: scaling x, A, B, dy (and the accumulator, bias and accumulated-onto gradients to match) by powers of
 *     two shifts every output by the sum of the exponents, bit for bit, as long as operands, stored intermediates and
 *     outputs stay in the normal range of the dtype and no non-zero term of a sum is below 2^-103 (fp32 on the split:
 *     2^-72);
 *   - non-finite values: a NaN or Inf inside x, dy or A makes non-finite exactly the output elements IEEE arithmetic makes
 *     non-finite (the row of y and h_save and the rows of dA of a poisoned token of x, ...); every other element is
 *     bit-identical to the run without it: zero padding never multiplies data of another token, layer or sibling.  bf16 /
 *     f16: an Inf that no other Inf cancels comes out as that Inf.  SOW_DTYPE_F32 on the 3 x bf16 split: an Inf operand
 *     yields NaN (the residual planes are Inf - Inf): only the set of non-finite elements is specified.  One exception: the kernels read a row of A
 *     together with the up to 64 elements that follow it in storage, against explicit zeros of dh, so a non-finite
 *     A[i, j] -- which makes all of y non-finite anyway -- may also make non-finite the columns i' < i of dx whose
 *     64-element window reaches it, (i - i') * r_live + j < 64, where IEEE arithmetic touches column i only;
 *   - subnormal operands are read at their value (the bf16 and f16 matrix pipe of gfx950 does not flush them; observed on
 *     every chain path), and subnormal outputs are kept.  SOW_DTYPE_F32 on the 3 x bf16 split: an fp32 value below 2^-110 may
 *     lose its mid / lo planes, which fall below the bf16 range -- an error of at most |x_k| |a_k| per such term;
 *   - `stream` is a hipStream_t passed as void* (0 = default stream); kernels are
 *     enqueued on it, so the calls are capturable into a hipGraph;
 *   - n_iter > 1 is presented as concatenated factors A = [A_1 .. A_n] ([d_in, n*r]),
 *     B = [B_1; ..; B_n] ([n*r, d_out]); sum_i A_i B_i = A B.
 */
#ifndef SOW_AMD_H
#define SOW_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SOW_DTYPE_F32 0
#define SOW_DTYPE_BF16 1
#define SOW_DTYPE_F16 2

/* Parameters in fp32 (mixed precision, as under torch.autocast): OR-ed into SOW_DTYPE_BF16 or SOW_DTYPE_F16 (the compute
 * dtype).  Accepted by sow_workspace_bytes, sow_forward_workspace_bytes, sow_forward, sow_backward, sow_backward_ex,
 * sow_backward_reduce_desc, sow_reduce_batch, sow_forward_group, sow_backward_group, sow_backward_group_reduce_desc and
 * sow_backward_group_plan; sow_forward_shared and sow_backward_shared return SOW_ERR_UNSUPPORTED for it (nothing launched:
 * the caller takes the grouped calls); every other entry point, and SOW_DTYPE_F32 | SOW_PARAM_F32 anywhere, returns
 * SOW_ERR_DTYPE (checked on the host before anything is launched or dereferenced).  With the flag:
 *   - the activations are of the compute dtype: x, y, h_save, dy, dx (and the internal dh);
 *   - A, B, bias, acc_down and acc_up (the accumulator unless SOW_ACC_NATIVE, below, says otherwise) are read as fp32, each element rounded once, to nearest even, to the compute dtype
 *     before use (the cast autocast applies to every F.linear / matmul operand, bias included): one launch packs all of
 *     them (every layer of a group call) into the caller's workspace, and the bf16 / f16 kernels run on the packed copies
 *     -- results equal those of the unflagged call on pre-rounded parameters bit for bit;
 *   - dA, dB and dbias are fp32, written as g = grad_beta * g + new, `new` the fp32 sum of the slab partials rounded once to
 *     fp32 (never through a bf16 / f16 intermediate); T = 0 zeroes fp32-sized gradients;
 *   - the workspace queries include the packed parameters: pass the flagged dtype to them.  The forward figure is then never
 *     0; it is the unflagged forward figure plus the packed parameters (a forward that needs no scratch of its own asks for
 *     the packed parameters only).  Nothing is cached between calls -- the parameters are packed again by every call that reads them (forward and
 *     the DATA phase of backward) -- and the calls stay capturable (no host synchronisation, no allocation). */
#define SOW_PARAM_F32 0x100

/* Permission to fuse a low-rank accumulator with the live term: OR-ed into the dtype like SOW_PARAM_F32.  The library MAY
 * then compute the SOW_ACC_LOWRANK term and the live term of a layer in one pass over the token rows (chain_wide_acc.hip)
 * instead of one chain launch per term.  It acts in sow_forward, in the SOW_BWD_DATA phase of sow_backward /
 * sow_backward_ex, in the per-layer fall-through of sow_forward_group / sow_backward_group, and in sow_workspace_bytes /
 * sow_forward_workspace_bytes, and it admits sibling sets with low-rank accumulators to the SOW_BWD_DATA phase of
 * sow_backward_shared (see there); every other entry point that takes a dtype accepts the flag and ignores it.  It is a
 * permission, never a demand: a flagged call outside the admitted set runs exactly what the unflagged call runs and returns
 * what it returns (never SOW_ERR_UNSUPPORTED because of the flag).  Admitted:
 *   - compute dtype bf16 or f16 WITHOUT SOW_PARAM_F32 (with it the permission is ignored);
 *   - SOW_ACC_LOWRANK, even r_live in [2, 64], even r_acc >= 2, r_acc + r_live <= 256, d_in and d_out multiples of 8;
 *   - at call time: 16-byte-aligned x / y / dY / dX / bias / h_save, a workspace of at least the FLAGGED query (which is the
 *     unflagged plan with a factor-pack region for r_acc + r_live columns, so a flagged workspace also serves the unflagged
 *     call; sow_forward_workspace_bytes is non-zero for an admitted flagged shape), and the NO_FUSED_ACC switch off.  The
 *     queries are pure functions of (shape, dtype with flags): NO_FUSED_ACC does not change them.
 * Rounding contract of the fused pass (u = the compute dtype's rounding, products and sums in fp32):
 *   forward   h_acc = rn(x Q), h_live = rn(scale * x A) = h_save (the r_live <= 64 layout), y = rn(h_acc R + h_live B + bias);
 *   backward  dh_acc = rn(dY R^T), dh_live = rn(scale * dY B^T) = dh (the workspace, as the two-pass path leaves it),
 *             dX = rn(dh_acc Q^T + dh_live A^T).
 * The projections are the values the unflagged path rounds; y / dX are rounded ONCE (the unflagged path rounds the
 * accumulator term to y / dX and adds the live term with a second rounding).  Fixed summation order: repeatable bits.  The
 * weight-gradient phases are the unflagged ones; they read h_save and dh as written here. */
#define SOW_FUSE_ACC 0x200

/* The same permission for low-rank accumulators past the 256 columns of SOW_FUSE_ACC: a second bit, OR-ed into the dtype next
 * to it (a caller may pass both; the two admitted sets are disjoint by r_acc + r_live, and SOW_FUSE_ACC keeps its set and its
 * workspace plan whatever this bit says).  The library MAY then run the SOW_ACC_LOWRANK term and the live term in one pass
 * whose H columns are computed in groups of 256 and kept on chip (chain_deep_acc.hip), instead of two generic GEMM launches
 * through a [T, r_acc] intermediate followed by the live chain with beta = 1.  It acts in sow_forward, in the SOW_BWD_DATA
 * phase of sow_backward / sow_backward_ex, in the per-layer fall-through of sow_forward_group / sow_backward_group and in
 * sow_workspace_bytes / sow_forward_workspace_bytes; every other entry point that takes a dtype, sow_forward_shared and
 * sow_backward_shared included, accepts the bit and ignores it.  A permission, never a demand, as SOW_FUSE_ACC.  Admitted:
 *   - compute dtype bf16 or f16 WITHOUT SOW_PARAM_F32 (with it the permission is ignored);
 *   - SOW_ACC_LOWRANK with both factors, even r_live in [2, 64], even r_acc, 256 < r_acc + r_live <= 960 (160 KiB of LDS:
 *     128 bytes per column of ceil64(r_acc + r_live) and a 40 KiB stage), d_in and d_out multiples of 8;
 *   - at call time: 16-byte-aligned x / y / dY / dX / bias / h_save, a workspace of at least the FLAGGED query (the unflagged
 *     plan, the [T, r_acc] scratch of the generic path included, with a factor-pack region for r_acc + r_live columns: it also
 *     serves the unflagged call), and the NO_DEEP_ACC switch off.  The queries do not depend on the switch.
 * Rounding contract, results (h_save, dh, y, dX) and the weight-gradient phases: those of SOW_FUSE_ACC above -- the bias is
 * added in fp32 before the one rounding of y. */
#define SOW_FUSE_ACC_DEEP 0x400

/* The accumulator of a SOW_PARAM_F32 call is already of the compute dtype (fp32 master factors over a frozen bf16 / f16 base,
 * or over the image of a quantised one): OR-ed into the dtype next to SOW_PARAM_F32.  With  cd | SOW_PARAM_F32 | SOW_ACC_NATIVE:
 *   - A, B and bias are fp32 and are packed exactly as under SOW_PARAM_F32;
 *   - acc_down / acc_up are tensors OF THE COMPUTE DTYPE, read in place by the kernels that read them in an unflagged call:
 *     never packed, never copied;
 *   - the workspace queries return the unflagged plan plus the 256-aligned packs of A, B and bias only (SOW_PARAM_F32's figure
 *     minus the packs of the accumulator tensors; the same figure for SOW_ACC_NONE);
 *   - y, h_save, dx and the internal dh are bit-identical to the unflagged call on parameters pre-rounded to the compute dtype,
 *     and to the SOW_PARAM_F32 call whose fp32 accumulator holds the same values; dA, dB and dbias are fp32 as under
 *     SOW_PARAM_F32.
 * Admitted: every entry point that accepts SOW_PARAM_F32 accepts the pair (sow_workspace_bytes, sow_forward_workspace_bytes,
 * sow_forward, sow_backward, sow_backward_ex, sow_backward_reduce_desc, sow_reduce_batch, sow_forward_group, sow_backward_group,
 * sow_backward_group_reduce_desc, sow_backward_group_plan), and sow_forward_skinny admits the pair although it refuses
 * SOW_PARAM_F32 alone (see there).  Without SOW_PARAM_F32 the bit is accepted wherever SOW_PARAM_F32 is accepted and ignored
 * there: the accumulator is native already.  Wherever SOW_PARAM_F32 is refused or rejected (sow_forward_shared and
 * sow_backward_shared: SOW_ERR_UNSUPPORTED; the entry points outside the layer surface: SOW_ERR_DTYPE) the bit gets the same
 * code, with or without SOW_PARAM_F32.  SOW_DTYPE_F32 with either flag stays SOW_ERR_DTYPE; SOW_FUSE_ACC* stay ignored next
 * to SOW_PARAM_F32.  The weight-gradient phases, plans and reduce descriptors read no accumulator: the bit changes nothing
 * there. */
#define SOW_ACC_NATIVE 0x800

#define SOW_OK 0
#define SOW_ERR_NULL (-1)
#define SOW_ERR_SHAPE (-2)
#define SOW_ERR_DTYPE (-3)
#define SOW_ERR_ALIGN (-4)
#define SOW_ERR_WORKSPACE (-5)
#define SOW_ERR_UNSUPPORTED (-6)

/* accumulator kinds of SoWLinear.forward (sow.py:109-112) */
#define SOW_ACC_NONE 0    /* acc_downweight empty                                   */
#define SOW_ACC_LOWRANK 1 /* out = (x @ acc_down[d_in,vr]) @ acc_up[vr,d_out]       */
#define SOW_ACC_DENSE 2   /* out = x @ acc_down[d_in,d_out]                         */
/* A frozen dense accumulator stored as OCP E4M3 codes with one power-of-two exponent per column:
 *   acc_down = the codes q [d_in, d_out], row-major, one byte each (e4m3fn; the two NaN codes are never produced),
 *   acc_up   = the exponents e [d_out], int8: the smallest e_n with max_k |W[k,n]| <= 448 * 2^e_n, clamped to [-117, 119]
 *              (bf16) or [-15, 7] (f16), 0 for an all-zero column;  q[k,n] = e4m3_rne(clamp(W[k,n] * 2^-e_n, -448, 448)).
 * The layer computes what SOW_ACC_DENSE computes on the dequantised matrix  W^[k,n] = q[k,n] * 2^e_n,  which inside those
 * clamps is exactly a number of the compute dtype: no rounding is added anywhere.  d_in * d_out + d_out bytes instead of
 * 2 * d_in * d_out.  sow_forward_skinny streams the codes as they are; every other layer entry point returns
 * SOW_ERR_UNSUPPORTED for this kind before anything is launched or dereferenced (the caller runs it on the image that
 * sow_acc_dequantize writes, with SOW_ACC_DENSE). */
#define SOW_ACC_DENSE_FP8 3
/* A frozen dense accumulator stored as MXFP4: E2M1 codes with one power-of-two scale per block of 32 consecutive rows k of one
 * column n (the MX block along the reduction dimension).  d_in a multiple of 32, d_out of 8.
 *   acc_up   = the block scales [d_in / 32, d_out], row-major, one E8M0 byte  e + 127  each:  e[kb, n] is the smallest integer
 *              with  max_{k in block} |W[k,n]| <= 6 * 2^e,  clamped to [-125, 125] (bf16) or [-13, 13] (f16), 0 for an all-zero
 *              block; the byte lies in [2, 252] (255, the E8M0 NaN, never occurs) and  byte << 23  is the fp32 scale;
 *   acc_down = the codes [d_in / 2, d_out], row-major:  byte[k / 2, n] = code(k, n) | code(k + 1, n) << 4  for even k, with
 *              code(k, n) = e2m1_rne(clamp(W[k,n] * 2^-e, -6, 6)),  values +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}, ties to the even
 *              code, the sign kept (-0 codes occur).
 * The layer computes what SOW_ACC_DENSE computes on  W^[k,n] = code(k, n) * 2^e[k / 32, n],  which inside those clamps is
 * exactly a (normal or zero) number of the compute dtype: no rounding is added anywhere.  (0.5 + 1/32) * d_in * d_out bytes.
 * sow_forward_skinny streams the codes as they are; every other layer entry point returns SOW_ERR_UNSUPPORTED for this kind
 * before anything is launched or dereferenced, and its workspace queries return 0 (the caller runs it on the image that
 * sow_acc_dequantize_fp4 writes, with SOW_ACC_DENSE). */
#define SOW_ACC_DENSE_FP4 4

#define SOW_H_COLS 64 /* column count of the saved h / dh buffers when r_live <= 64 */

int sow_version(void);
const char* sow_error_string(int code);

/* Kernel-selection switches -- for A/B measurements and for the tests that pin every kernel variant; production code
 * never touches them.  They are the library's ONLY process-wide state: a table of atomics initialised from the
 * environment (SOW_AMD_<NAME>) once, at first use; no launch path calls getenv.  Names: FORCE_CHAIN_V1, NO_SHORT_SPLIT,
 * NO_FUSED_H, FORCE_GEMM_V1, TN_NARROW, NO_GEMM3S, NO_GROUPED, NO_PERSIST, NO_NT_STORE, NT_LOAD, NO_PAIR_FLUSH, F32_EXACT, NO_PARK16, TN_NO_NT_LOAD, NO_TN_ROWS, NO_GEMM4H, NO_CHAIN3F, NO_TN_F32Q, NO_SPLITK,
 * NO_WIDE_CHAIN, NO_SHARED_X, NO_RAGGED, NO_RAGGED_GEMM, NO_BLOCKED_QR, NO_SKINNY, NO_H_ROWS, NO_X_PAIR, NO_FUSED_ACC, NO_DEEP_ACC
 * (value 1 = on, -1 / 0 = off), NO_ROW_ALIGN (1 = on, 2 = on for the X stages only, 3 = on for the Y slices only; it keeps
 * and returns that value) and GEMM3S, GEMM3, GEMM4
 * (1 = force, 0 = forbid, -1 = automatic).  sow_set_switch returns SOW_ERR_UNSUPPORTED for an unknown name;
 * sow_get_switch returns the value (-1 / 0 / 1).  Changing a switch while other threads launch is safe (atomic) but
 * the launches in flight may see either value. */
int sow_set_switch(const char* name, int value);
int sow_get_switch(const char* name);

/* Bytes of workspace needed by sow_forward / sow_backward for this shape. */
size_t sow_workspace_bytes(int64_t T, int d_in, int d_out, int r_live, int r_acc, int acc_kind, int dtype);
/* Bytes of workspace sow_forward itself touches: 0 for most bf16 shapes (the caller may then pass NULL / 0), else the
 * same figure as sow_workspace_bytes (r_live > 64: the packed factors of the fused wide chain, or the projection when the
 * caller passes h_save = NULL to the generic composition; a low-rank accumulator wider than 64; short inputs, whose chain is split over K
 * and over the output columns to fill the chip; fp32 inputs with T >= 8192, whose factors are pre-split into bf16 planes
 * there; a bf16 dense accumulator at short T and long K, whose product is split over K).  A caller that passes NULL / 0
 * where the query is non-zero still gets the right result from a slower kernel, except for the wide low-rank accumulator
 * (SOW_ERR_WORKSPACE). */
size_t sow_forward_workspace_bytes(int64_t T, int d_in, int d_out, int r_live, int r_acc, int acc_kind, int dtype);
/* Elements (of dtype) the caller must allocate for h_save: T*64 when r_live <= 64, else T*r_live. */
size_t sow_h_save_elems(int64_t T, int r_live);

/* SoWLinear.forward -- replaces sow.py:107-126:
 *   y = acc_term + scale * (x @ A) @ B + bias,   h_save = scale * (x @ A) for r_live <= 64 (padded to 64
 *   columns, column 63 = 1.0 when free) or x @ A for r_live > 64 ([T, r_live] row-major, rounded once; y is computed from
 *   the rounded h); opaque to the caller, kept for backward.  h_save may be NULL when no backward follows (the projection
 *   then stays on chip, or goes to the workspace).
 * bf16 / f16 layers with even r_live in (64, 256], d_in and d_out multiples of 8 and 16-byte-aligned x / y / bias run the
 * fused wide chain (one pass over x; the NO_WIDE_CHAIN switch forces the generic GEMM composition), as does a low-rank
 * accumulator with even r_acc in (64, 256]; their backward runs the same chain for dX and a token-slab weight-gradient
 * kernel (dA, dB and dbias in one pass over x and dY, partial sums added in a fixed order).
 * Ragged widths: bf16 / f16 layers (SOW_PARAM_F32 included) with even r_live in (64, 256] and d_in or d_out NOT a multiple
 * of 8, with no accumulator, a dense one or a low-rank one of even r_acc in [2, 256], run the same two kernels with token
 * rows read and written at any 2-byte offset (x / y / dY / dX / bias bases still 16-byte aligned; the weight gradients take
 * any x / dY view).  A dense accumulator's products x W_acc and dY W_acc^T run on the ragged dense GEMM (gemm_rag.hip:
 * W_acc read in place at its own row pitch, no copy, rounded once) ahead of the chain, which adds the live term with
 * beta = 1; the NO_RAGGED_GEMM switch sends only that product to the generic GEMM.  Their workspace query covers the pack
 * and the slab partials whatever the NO_RAGGED / NO_RAGGED_GEMM switches say; NO_RAGGED (or a misaligned view) restores
 * the generic kernels.  Ranks <= 64 at ragged widths, r_acc > 256, odd ranks and fp32 layers keep the generic kernels.
 * x [T,d_in], A [d_in,r_live], B [r_live,d_out], y [T,d_out]; acc_down/acc_up per acc_kind
 * (r_acc = vr for SOW_ACC_LOWRANK, ignored otherwise); bias [d_out] or NULL.
 * The accumulator term is NOT scaled (sow.py:110-112). */
int sow_forward(const void* x, const void* A, const void* B, const void* acc_down, const void* acc_up, const void* bias,
                void* y, void* h_save, int64_t T, int d_in, int d_out, int r_live, int r_acc, int acc_kind, float scale,
                int dtype, void* workspace, size_t workspace_bytes, void* stream);

/* Backward of the above (what autograd derives from sow.py:107-126):
 *   dh = scale * dY @ B^T ; dB = scale * h^T @ dY ; dA = x^T @ dh ;
 *   dX = dh @ A^T + acc-term ; dbias = sum_t dY.
 * Gradients are written as  g = grad_beta * g + new  (grad_beta = 0 overwrites, 1 accumulates).
 * dbias may be NULL (no bias).  dx must be non-NULL. */
int sow_backward(const void* dy, const void* x, const void* h_save, const void* A, const void* B, const void* acc_down,
                 const void* acc_up, void* dx, void* dA, void* dB, void* dbias, int64_t T, int d_in, int d_out,
                 int r_live, int r_acc, int acc_kind, float scale, float grad_beta, int dtype, void* workspace,
                 size_t workspace_bytes, void* stream);

/* The same in two phases, so that the weight-gradient kernels (off the critical path of backpropagation)
 * can run on another stream than the data-gradient kernel:
 *   SOW_BWD_DATA    : dX and the internal dh = scale * dY @ B^T (kept in `workspace`)
 *   SOW_BWD_WEIGHTS : dA, dB, dbias from x, dY, h_save and the dh left in the SAME workspace by a
 *                     preceding SOW_BWD_DATA call (the caller orders the two calls, e.g. with an event).
 * SOW_BWD_WEIGHTS = SOW_BWD_WEIGHTS_PARTIAL (the token-slab partial sums, left in `workspace`) followed by
 * SOW_BWD_WEIGHTS_REDUCE (their fixed-order sum into dA / dB / dbias); the two may also be requested separately, e.g.
 * to run the small reduction beside the next layer's kernels (r_live <= 64; for wider ranks PARTIAL does everything
 * and REDUCE nothing).
 * phases = SOW_BWD_DATA | SOW_BWD_WEIGHTS is sow_backward. */
#define SOW_BWD_DATA 1
#define SOW_BWD_WEIGHTS 2
#define SOW_BWD_WEIGHTS_PARTIAL 4
#define SOW_BWD_WEIGHTS_REDUCE 8
/* sow_backward_group only: the token-slab counts of the weight-gradient partial sums may be planned over the whole group
 * (row-owner kernel, see sow_backward_group) although the reduction is deferred; the deferred reduction must then be
 * built with sow_backward_group_reduce_desc(same layers, same flag).  bf16: implied when one call runs PARTIAL and REDUCE;
 * f16: never implied (see sow_backward_group_reduce_desc below). */
#define SOW_BWD_GROUP_SLABS 16
int sow_backward_ex(const void* dy, const void* x, const void* h_save, const void* A, const void* B,
                    const void* acc_down, const void* acc_up, void* dx, void* dA, void* dB, void* dbias, int64_t T,
                    int d_in, int d_out, int r_live, int r_acc, int acc_kind, float scale, float grad_beta, int dtype,
                    void* workspace, size_t workspace_bytes, int phases, void* stream);

/* Deferred, batched reduction of the weight gradients.  A training step calls sow_backward_ex(phases = SOW_BWD_DATA |
 * SOW_BWD_WEIGHTS_PARTIAL) for every layer, each with its OWN workspace (the slab partials stay there), and sums all of
 * them in ONE launch before the gradients are consumed (optimizer step / all-reduce): one launch instead of one 5-us
 * launch per layer, same per-element summation order as SOW_BWD_WEIGHTS_REDUCE (bit-identical results).
 *   sow_reduce_desc_bytes()    size of one opaque descriptor
 *   sow_backward_reduce_desc() writes the descriptor of one layer to HOST memory `desc_out` and its block count to
 *                              `blocks_out` (same shape / pointer arguments as the sow_backward_ex call it completes;
 *                              r_live > 64: an empty descriptor with 0 blocks, PARTIAL already finished the gradients;
 *                              SOW_ERR_UNSUPPORTED for r_live = 64 with dbias: no separate reduction -- use
 *                              SOW_BWD_WEIGHTS); sow_reduce_batch skips 0-block entries
 *   sow_reduce_batch()         `descs`: n descriptors back to back in DEVICE memory; `starts`: n ints in device memory,
 *                              starts[i] = sum of the block counts of layers < i; total_blocks = their total. */
size_t sow_reduce_desc_bytes(void);
int sow_backward_reduce_desc(void* dA, void* dB, void* dbias, int64_t T, int d_in, int d_out, int r_live, int r_acc,
                             int acc_kind, float grad_beta, int dtype, void* workspace, size_t workspace_bytes, void* desc_out,
                             int* blocks_out);
int sow_reduce_batch(const void* descs, const int* starts, int n, int total_blocks, int dtype, void* stream);

/* Grouped calls: n INDEPENDENT SoWLinear invocations in as few launches as possible -- the q / k / v projections of
 * an attention block (sow.py:107-126 called three times on the same hidden state by the HF model), gate / up of an MLP,
 * and their backward passes.  Each element carries exactly the arguments of sow_forward / sow_backward_ex for its
 * layer (fields a direction does not use are ignored).  Semantics = the n single calls, in any order; results are
 * bit-identical to them.  Layers that run the bf16 / f16 streaming kernels (no accumulator, r_live <= 64, T > 8192) share one
 * grid per kernel, up to 4 layers at a time: a launch costs ~8 us of ramp + first-load latency + write drain whatever
 * its size, which a 3-layer grid pays once.  Every other layer is forwarded to the single-layer entry point. */
typedef struct sow_layer_args {
  const void* x;        /* [T, d_in]                                      */
  const void* A;        /* [d_in, r_live]                                 */
  const void* B;        /* [r_live, d_out]                                */
  const void* acc_down; /* per acc_kind, or NULL                          */
  const void* acc_up;
  const void* bias;     /* [d_out] or NULL                                */
  void* y;              /* forward output [T, d_out]                      */
  void* h_save;         /* sow_h_save_elems(T, r_live) elements           */
  const void* dy;       /* backward: upstream gradient [T, d_out]         */
  void* dx;             /* [T, d_in]                                      */
  void* dA;
  void* dB;
  void* dbias;          /* or NULL                                        */
  int64_t T;
  int32_t d_in, d_out, r_live, r_acc, acc_kind;
  float scale, grad_beta;
  void* workspace;      /* this layer's own workspace (sow_workspace_bytes) */
  size_t workspace_bytes;
} sow_layer_args;
int sow_forward_group(const sow_layer_args* layers, int n, int dtype, void* stream);
/* phases as in sow_backward_ex; the phases run in order DATA (all layers), WEIGHTS_PARTIAL (all), WEIGHTS_REDUCE (all). */
int sow_backward_group(const sow_layer_args* layers, int n, int dtype, int phases, void* stream);
/* Weight gradients of a group: with enough layers to fill the chip (e.g. the 7 projections of a llama decoder block) the
 * partial sums run in the ROW-OWNER kernel -- a workgroup owns all columns of a token slab, so h / dh are read once instead
 * of once per 128 columns and x / dY arrive as whole rows -- with slab counts planned over the group (equal work per
 * workgroup, one resident round; a pure function of the layer list).  The sums are then added in a different (still
 * fixed) order than by n single calls: dA / dB / dbias agree with them to fp32 rounding of the slab sums, not bit for bit.
 * SOW_DTYPE_BF16 and SOW_DTYPE_F16 (SOW_PARAM_F32 included) take this plan, with one deliberate asymmetry: f16 takes it ONLY
 * when the caller passes SOW_BWD_GROUP_SLABS (a deferred reduction, e.g. FactorBucket); an f16 call that runs PARTIAL and
 * REDUCE itself keeps the column-owner kernel and stays bit-identical to n single calls (bf16: the flag is implied there).
 * The NO_F16_TN switch sends every f16 weight gradient back to the generic kernel (no grouping, no row-owner plan).
 * sow_backward_group_reduce_desc: the descriptors (n x sow_reduce_desc_bytes(), HOST memory) and block counts of the
 * deferred reductions of exactly this group, for sow_reduce_batch; `phases` = the flags of the PARTIAL call. */
int sow_backward_group_reduce_desc(const sow_layer_args* layers, int n, int dtype, int phases, void* descs_out, int* blocks_out);
/* What sow_backward_group(layers, n, dtype, phases) does for the weight gradients: returns 1 if the row-owner kernel with
 * group-planned slabs runs, 0 if every layer keeps its single-layer slab count (negative: error); slabs_out (2 n ints,
 * may be NULL) receives the token-slab counts of the x / dY operand of every layer. */
int sow_backward_group_plan(const sow_layer_args* layers, int n, int dtype, int phases, int* slabs_out);

/* Shared-input calls: n <= 4 SIBLING layers on ONE input (q / k / v, gate / up), fused into one launch per direction.
 * The forward streams x once for all of them; the data gradient writes ONE dX for the set:
 *   dX = grad_beta * dX + sum_i dh_i @ A_i^T,   dh_i = scale_i * dY_i @ B_i^T,
 * summed in fp32 inside the kernel and rounded ONCE to the compute dtype (not the rounding of n separate dX added later).
 * Every layers[i].x must be the same pointer (else SOW_ERR_SHAPE), with one T and one d_in; d_out and r_live may differ.
 * layers[0].dx receives the sum with layers[0].grad_beta; every other dx must be NULL or equal to it (else SOW_ERR_SHAPE).
 * y_i, h_save_i and the dh_i the weight phases read are bit-identical to sow_forward_group / sow_backward_group on the same
 * inputs.  The weight phases in `phases` (BWD_WEIGHTS, _PARTIAL, _REDUCE, GROUP_SLABS) run exactly as sow_backward_group
 * runs them.  Admitted: bf16 or f16 (no SOW_PARAM_F32), SOW_ACC_NONE, r_live <= 64, T > 8192, the alignment of the
 * streaming kernels; anything else -- and everything while the NO_SHARED_X switch is on -- returns SOW_ERR_UNSUPPORTED,
 * and then nothing has been launched (the caller runs sow_forward_group / sow_backward_group instead).
 *
 * SOW_FUSE_ACC in the dtype of sow_backward_shared admits a second set to its SOW_BWD_DATA phase: siblings that ALL carry a
 * low-rank accumulator (chain_shared_acc.hip: the fused chains of the siblings over one token block, their dX summed on
 * chip; a factor pack launch and one kernel launch whatever n).  Tested where the set above is refused, after every check
 * before it.  Admitted when all of these hold:
 *   - compute dtype bf16 or f16, SOW_FUSE_ACC without SOW_PARAM_F32, n <= 4, T > 8192;
 *   - every sibling SOW_ACC_LOWRANK (both factors given) in the admitted set of SOW_FUSE_ACC: even r_live in [2, 64], even
 *     r_acc >= 2, r_acc + r_live <= 256, d_in and d_out multiples of 8;
 *   - the LDS plan fits into 160 KiB: with r_pad_i = ceil64(r_acc_i + r_live_i),
 *       128 * sum_i r_pad_i + max(128 * max_i r_pad_i + 8192, 24576) bytes
 *     (three siblings of r_pad = 256 plan 136 KiB; the largest admitted set is r_pad = 256, 256, 256, 192: 15 panels of 64
 *     columns, exactly 160 KiB; four of 256 do not fit; q / k / v at r_pad = 128 plan 72 KiB: two workgroups per CU);
 *   - every dY_i, dX and every dh_i (the workspaces) 16-byte aligned;
 *   - every sibling's workspace at least its FLAGGED sow_workspace_bytes;
 *   - the NO_SHARED_X and NO_FUSED_ACC switches off.
 * Any other set returns SOW_ERR_UNSUPPORTED with nothing launched and nothing written, as before: an unflagged dtype, a set
 * mixed with SOW_ACC_NONE or dense siblings, a workspace between the unflagged and the flagged plan (the permission the
 * caller cannot use: sow_backward_group runs it).  A workspace below the UNFLAGGED plan of an otherwise admitted set is
 * SOW_ERR_WORKSPACE.  A call without SOW_BWD_DATA is unchanged.
 * Contract (u = the compute dtype's rounding, products and sums in fp32):
 *   dh_acc_i = rn(dY_i R_i^T), dh_live_i = rn(scale_i * dY_i B_i^T) = dh_i, written where and as the single fused pass writes
 *   it ([T, 64], zeros above r_live, 1.0 in column 63 when r_live < 64): each dh_i the weight phases read is bit-identical
 *   to a sow_backward_group call flagged with SOW_FUSE_ACC on the same inputs, and so are dA, dB and dbias from it;
 *   dX = rn(grad_beta * dX + sum_i (dh_acc_i Q_i^T + dh_live_i A_i^T)): ONE fp32 accumulation -- sibling 0's columns in
 *   ascending order, then sibling 1's, ... -- and ONE rounding.  No atomics: a repeated call gives the same bits.
 * sow_forward_shared keeps refusing low-rank sets, flagged or not: the shared forward measured no gain even without an
 * accumulator (q + k + v 43.2 against 42.4 us grouped), and a phase 1 over the siblings' sum_i r_pad_i columns side by side
 * -- what reading x once would take -- has no room in the register file (r_pad = 256 of ONE sibling fills the accumulators). */
int sow_forward_shared(const sow_layer_args* layers, int n, int dtype, void* stream);
int sow_backward_shared(const sow_layer_args* layers, int n, int dtype, int phases, void* stream);

/* Generation-sized forwards: n <= 16 INDEPENDENT layers of at most 32 tokens each (the per-token calls of generate(): T =
 * batch x beams; q / k / v or gate / up of a decoder block in one call) in TWO launches, whatever n:
 *   h = rn( scale * sum_k x[t,k] A[k,j] )                                  fp32 sum, rounded once to the compute dtype
 *   y = rn( sum_k x[t,k] acc_down[k,n] + sum_j h[t,j] B[j,n] + bias[n] )   fp32 sum, rounded ONCE
 * (the h of the r_live <= 64 contract, never written to memory here; the single output rounding of the training forward's
 * fused dense product).  The first launch streams the accumulator once on the whole chip -- a grid over column ranges x
 * K-slabs -- and leaves fp32 slab partials of x . acc_down and x . A in the workspace; the second adds them in slab order
 * with h . B and the bias.  No atomics: a repeat gives the same bits, and a layer computes inside a group exactly what it
 * computes alone.  Rows are independent: a non-finite x[t, k] makes row t of y non-finite and no other.
 * Fields used: x, A, B, acc_down, bias, y, T, d_in, d_out, r_live, acc_kind, scale, workspace, workspace_bytes (h_save and
 * the backward fields are ignored).  Layers may share x or not.
 * Admitted: SOW_DTYPE_BF16 / SOW_DTYPE_F16, T <= 32, SOW_ACC_DENSE, SOW_ACC_DENSE_FP8, SOW_ACC_DENSE_FP4 or SOW_ACC_NONE, r_live <= 64,
 * d_in and d_out multiples of 8 (d_in of 32 with SOW_ACC_DENSE_FP4), 16-byte-aligned x, y, acc_down, A, B and bias, n <= 16.  Anything else -- SOW_ACC_LOWRANK, SOW_PARAM_F32
 * without SOW_ACC_NATIVE, and everything while the NO_SKINNY switch is on -- returns SOW_ERR_UNSUPPORTED; SOW_DTYPE_F32 returns SOW_ERR_DTYPE and a
 * workspace below the query SOW_ERR_WORKSPACE.  All of it is decided on the host for every layer before anything is launched
 * or dereferenced (the caller then takes sow_forward / sow_forward_group).  Layers with T = 0 are skipped (SOW_OK).
 * sow_forward_skinny_workspace_bytes: per layer, a pure function of the shape (the switches do not enter); 0 outside the
 * admitted set.  Every scratch byte is written before it is read.
 * SOW_ACC_DENSE_FP8 (acc_down = codes, acc_up = exponents, 8-byte aligned): the first launch reads the codes as bytes --
 * half the stream -- converts them unscaled in registers and leaves sum_k x[t,k] q[k,n] in the slab partials; the second
 * multiplies their slab-order sum by 2^e_n in fp32 (exact) before h . B and the bias: y = rn(x W^ + h B + bias), one
 * rounding, the contract above with acc_down := W^.  Its column ranges are 128 wide, so its slab plan and workspace differ
 * from SOW_ACC_DENSE's: size the workspace of such a layer with sow_forward_skinny_fp8_workspace_bytes (below).  The dense layers of one call must all be of one kind (SOW_ERR_UNSUPPORTED otherwise; layers without
 * an accumulator mix with either).
 * SOW_ACC_DENSE_FP4 (acc_down = packed codes, acc_up = E8M0 block scales, both 8-byte aligned): the first launch reads a
 * quarter of the stream -- 8-byte pieces of 8 columns x 2 rows, and the block's 8 scale bytes once per 32 rows -- and converts a
 * byte and its scale straight into an MFMA operand register (v_cvt_scalef32_pk_{bf16,f16}_fp4: exact); the slab partials
 * hold sum_k x[t,k] W^[k,n] and the second launch is the one of SOW_ACC_DENSE.  128-column ranges as for SOW_ACC_DENSE_FP8;
 * size the workspace with sow_forward_skinny_fp4_workspace_bytes.  Kinds 2, 3 and 4 do not mix in one call.
 * fp32 factors: dtype = cd | SOW_PARAM_F32 | SOW_ACC_NATIVE is admitted for all four kinds, every other condition unchanged (A,
 * B and bias of every layer are then fp32, 16-byte aligned; the accumulator is of cd, or codes).  No pack launch and no extra
 * workspace -- the three queries answer for the flagged dtype what they answer for cd (and 0 for SOW_PARAM_F32 alone): the x . A
 * workgroups of the first launch gather A with 4-byte loads, the second loads its column of B and the bias as fp32, and each
 * value is rounded once, to nearest even, to cd in registers before use.  y is bit-identical to the unflagged call on factors
 * pre-rounded to cd.  SOW_ACC_NATIVE alone is ignored (the unflagged call). */
size_t sow_forward_skinny_workspace_bytes(int64_t T, int d_in, int d_out, int r_live, int acc_kind, int dtype);
/* The same query for a layer with SOW_ACC_DENSE_FP8, under the conditions of SOW_ACC_DENSE (0 outside them).  A query of
 * its own: sow_forward_skinny_workspace_bytes answers 0 for acc_kind = 3, as it did while 3 was no kind, so that a caller
 * written against it keeps reading 3 as "not admitted" there. */
size_t sow_forward_skinny_fp8_workspace_bytes(int64_t T, int d_in, int d_out, int r_live, int dtype);
/* The same for SOW_ACC_DENSE_FP4 (0 outside SOW_ACC_DENSE's conditions or when d_in is no multiple of 32); the query above
 * answers 0 for acc_kind = 4 for the same reason. */
size_t sow_forward_skinny_fp4_workspace_bytes(int64_t T, int d_in, int d_out, int r_live, int dtype);
int sow_forward_skinny(const sow_layer_args* layers, int n, int dtype, void* stream);

/* The same forward for up to SOW_SKINNY_ROWS_MAX tokens per layer (decode steps of batch x beams = 33 ... 64, e.g. 16 prompts
 * x 4 beams): the same contract, the same two launches, every byte of the accumulator (codes, scales) still read once.  A
 * layer with 33 <= T <= 64 takes instantiations of the same two kernels that hold three or four 16-row tiles per wave -- each
 * fragment of W is built or converted once and fed to up to four MFMAs -- and a slab plan of its own (fewer, longer slabs:
 * the fp32 slab partials grow with T).  A layer with T <= 32 takes the plan and the kernels of sow_forward_skinny and gives
 * the same bits, also next to a 64-row layer in one call (layers of both ranges are then launched as two groups).
 * Admitted: 1 <= T <= 64 per layer, every other condition as for sow_forward_skinny: bf16 / f16 (SOW_PARAM_F32 only with
 * SOW_ACC_NATIVE), SOW_ACC_NONE / _DENSE / _DENSE_FP8 / _DENSE_FP4 (the dense kinds do not mix in a call), r_live <= 64, widths
 * multiples of 8 (d_in of 32 for _DENSE_FP4), the alignments, n <= 16; the same return codes, decided on the host for every
 * layer before anything is launched or dereferenced; NO_SKINNY refuses everything; layers with T = 0 are skipped.
 * sow_forward_skinny_rows_workspace_bytes: ONE query for all four kinds, a pure function of the shape, 0 outside the admitted
 * set; for T <= 32 it returns what the matching query above returns.  Every scratch byte is written before it is read. */
#define SOW_SKINNY_ROWS_MAX 64
size_t sow_forward_skinny_rows_workspace_bytes(int64_t T, int d_in, int d_out, int r_live, int acc_kind, int dtype);
int sow_forward_skinny_rows(const sow_layer_args* layers, int n, int dtype, void* stream);

/* Short batches of dense-accumulator layers, WITH gradients: n <= 16 independent layers of 1 ... SOW_SHORT_ROWS_MAX rows each on
 * the two skinny kernels, cut into row blocks of 64 on one W (one launch pair per 16 (layer, row block) entries):
 *   forward   h   = rn(scale * x A)              fp32 sum, rounded once  -> h_save (the r_live <= 64 layout) when given
 *             y   = rn(x acc_down + h B + bias)  ONE fp32 sum, rounded once
 *   data      dh  = rn(scale * dY B^T)           fp32 sum, rounded once  -> the workspace, where the weight phases read it
 *             dX  = rn(dY acc_down^T + dh A^T)   ONE fp32 sum, rounded once
 * h_save and dh have the layout the streaming kernels leave: [T][64], zeros past r_live, 1.0 in column 63 when r_live <= 63.
 * sow_backward_short runs the data phase only; an unchanged sow_backward_ex(..., SOW_BWD_WEIGHTS | _PARTIAL | _REDUCE) on the
 * same workspace then produces dA, dB and dbias.  acc_down is read in place in both directions (transposed by the loads of
 * the data phase).  No atomics and a fixed order of every sum: a repeat gives the same bits, a layer computes inside a call what
 * it computes alone, and a row's result does not depend on its position or on the rows next to it.
 * Fields used: forward x, A, B, acc_down, bias, y, h_save (may be NULL); data phase dy, A, B, acc_down, dx; both T, d_in,
 * d_out, r_live, acc_kind, scale, workspace, workspace_bytes.
 * Admitted: SOW_DTYPE_BF16 / SOW_DTYPE_F16 without flags, SOW_ACC_DENSE only, 1 <= T <= SOW_SHORT_ROWS_MAX, r_live <= 64, d_in and
 * d_out multiples of 8, 16-byte-aligned x, y, dy, dx, acc_down, A, B, bias and h_save, n <= 16.  SOW_ACC_NONE, SOW_ACC_LOWRANK,
 * the code kinds, SOW_PARAM_F32 (with or without SOW_ACC_NATIVE) and everything while the NO_SKINNY switch is on return
 * SOW_ERR_UNSUPPORTED; SOW_DTYPE_F32 returns SOW_ERR_DTYPE; a workspace below the query SOW_ERR_WORKSPACE.  All of it is decided
 * on the host for every layer before anything is launched or dereferenced.  Layers with T = 0 are skipped (SOW_OK).
 * sow_forward_short_workspace_bytes: the forward's slab partials (a no-grad call needs no more).
 * sow_short_workspace_bytes: ONE size for the forward, the data phase and the weight phases -- the plan of sow_workspace_bytes
 * for the same layer with the 256-aligned slab partials appended, so the buffer passes sow_backward_ex's size check and dh sits
 * where that plan keeps it.  (The forward writes its partials to the front of the workspace it is given: nothing there is live
 * before the data phase.)  Both are pure functions of the shape, 0 outside the admitted set; every byte of the partials is
 * written before it is read. */
#define SOW_SHORT_ROWS_MAX 1024
size_t sow_forward_short_workspace_bytes(int64_t T, int d_in, int d_out, int r_live, int acc_kind, int dtype);
size_t sow_short_workspace_bytes(int64_t T, int d_in, int d_out, int r_live, int acc_kind, int dtype);
int sow_forward_short(const sow_layer_args* layers, int n, int dtype, void* stream);
int sow_backward_short(const sow_layer_args* layers, int n, int dtype, void* stream);

/* The same on a quantised accumulator READ IN PLACE: acc_down = the codes, acc_up = the scales (as in sow_forward_skinny), no image
 * and no arena traffic.  The contract is the one above with acc_down := W^, the matrix sow_acc_dequantize / sow_acc_dequantize_fp4
 * write for the same codes and scales:
 *   forward   y  = rn(x W^ + h B + bias)          data   dX = rn(dY W^T + dh A^T)
 * with h, dh, h_save, the workspace layout, the order of every sum and the invariants as above.  The data phase dequantises in
 * registers to the exact bits of W^ and keeps the geometry of sow_backward_short: dX and dh are bit-identical to sow_backward_short on the
 * image.  The weight phases are an unchanged sow_backward_ex(..., SOW_BWD_WEIGHTS ...) on the same workspace, called with acc_kind =
 * SOW_ACC_DENSE (they read no accumulator); the workspace is sized for that plan.
 * Admitted: acc_kind SOW_ACC_DENSE_FP8 or SOW_ACC_DENSE_FP4 only, all layers of a call of ONE kind; SOW_DTYPE_BF16 / SOW_DTYPE_F16
 * without flags; 1 <= T <= SOW_SHORT_ROWS_MAX, r_live <= 64, n <= 16; E4M3: d_in and d_out multiples of 8, 16-byte-aligned codes, 8-byte-aligned
 * exponents (the data phase loads eight at once); MXFP4: d_in a multiple of 32, d_out of 8, 8-byte-aligned codes and scales; the other operands
 * aligned as above.  SOW_ACC_DENSE, SOW_ACC_NONE, SOW_ACC_LOWRANK, mixed code kinds, more than 16 layers, SOW_PARAM_F32 and everything while NO_SKINNY is
 * on return SOW_ERR_UNSUPPORTED; the other codes are those of sow_forward_short; all decided on the host for every layer before a launch
 * or a dereference.  The queries are pure functions of the shape (no switch moves them) and 0 outside the admitted set;
 * sow_short_codes_workspace_bytes = the plan of sow_workspace_bytes(..., SOW_ACC_DENSE, ...) with the larger direction's slab partials
 * appended, sow_forward_short_codes_workspace_bytes = the forward's partials alone. */
size_t sow_forward_short_codes_workspace_bytes(int64_t T, int d_in, int d_out, int r_live, int acc_kind, int dtype);
size_t sow_short_codes_workspace_bytes(int64_t T, int d_in, int d_out, int r_live, int acc_kind, int dtype);
int sow_forward_short_codes(const sow_layer_args* layers, int n, int dtype, void* stream);
int sow_backward_short_codes(const sow_layer_args* layers, int n, int dtype, void* stream);

/* General row-major GEMM  C[M,N] = alpha * op(A) op(B) + beta * C + bias[N]  (bias may be NULL).
 * trans_a: A is stored [K,M]; trans_b: B is stored [N,K].  Replaces the plain `@` / einsum call
 * sites: accumulate() sow.py:131-140 (W_acc += scale * A @ B, Q @ R), prepare.py:135, tt.py:213-237. */
int sow_gemm(const void* A, int64_t lda, int trans_a, const void* B, int64_t ldb, int trans_b, void* C, int64_t ldc,
             const void* bias, int64_t M, int N, int K, float alpha, float beta, int dtype, void* stream);

/* The same with scratch for the caller's stream: short bf16 products (M <= ~1024 rows of a wide output: fewer output tiles
 * than the chip has CUs) are split over K across workgroups, fp32 partial sums through `workspace`, summed in a fixed
 * order.  sow_gemm_workspace_bytes returns 0 when the shape does not split (workspace may then be NULL); sow_gemm is
 * sow_gemm_ex without scratch. */
size_t sow_gemm_workspace_bytes(int64_t M, int N, int K, int trans_a, int dtype);
int sow_gemm_ex(const void* A, int64_t lda, int trans_a, const void* B, int64_t ldb, int trans_b, void* C, int64_t ldc,
                const void* bias, int64_t M, int N, int K, float alpha, float beta, int dtype, void* workspace,
                size_t workspace_bytes, void* stream);

/* Truncated Householder QR -- replaces qr_weight (utils.py:8-30) and the truncated complete-mode QR
 * of TensorTrain.decompose (tt.py:128-136):  Q_out[m,k] = Q[:, :k], R_out[k,n] = R[:k, :]
 * with LAPACK's sign convention.  W [m,n] (ldw) of in_dtype; outputs of out_dtype; internals fp32.
 * R_out may be NULL (sow.py:168-172 only needs Q).  k <= m.  For n < k only n columns are factored: Q_out[:, :n] is the
 * reduced Q (all that qr_weight returns), Q_out[:, n:k] the complete-mode columns H_0 .. H_{n-1} e_j, R_out rows n.. are 0.
 * Up to 64 factored columns (kc = min(k, m, n)) one workgroup runs the unblocked panel; wider panels are factored by blocks
 * of 32 columns (compact WY, qr_blocked.hip): the block on one workgroup, its trailing update and the formation of Q on
 * the whole chip, same signs and taus, results repeatable bit for bit.  The NO_BLOCKED_QR switch keeps the one-workgroup
 * panel at every width.  Both routes hold a reflector of m floats in LDS: SOW_ERR_UNSUPPORTED past about 38400 rows.  The workspace query is a pure function of the shape: it covers the blocks' triangular factors
 * whenever kc > 64, whatever the switch says. */
size_t sow_qr_workspace_bytes(int m, int n, int k, int in_dtype, int need_r);
int sow_qr_thin(const void* W, int64_t ldw, int m, int n, int in_dtype, int k, void* Q_out, int64_t ldq, void* R_out,
                int64_t ldr, int out_dtype, void* workspace, size_t workspace_bytes, void* stream);

/* The periodic step of MANY layers -- replaces the loop of tn_gradient/prepare.py:219-222 over
 * SoWLinear.accumulate (sow.py:128-178) for layers on the dense-accumulator branch (the one every script takes:
 * prepare.py:120 forces virtual_rank = min(in, out)).  Per item, in stream order:
 *     acc   = acc_beta * acc + scale * A . B          (sow.py:131-140; acc_beta = 0 materialises a first accumulator)
 *     A_new = Q[:, :r_new] of the Householder QR of `draw` [d_in, draw_cols]   (sow.py:161-172; skipped when draw = NULL)
 *     `zero` buffer <- 0                                (B <- 0, sow.py:159)
 * One launch per phase for all items (the per-layer QR panel is latency-bound on one CU; n of them run side by side).
 * A_new may alias A: it is written after the update has consumed A.  Workspace per item:
 * sow_qr_workspace_bytes(d_in, draw_cols, r_new, dtype, 0).  r <= 64. */
typedef struct sow_accumulate_args {
  void* acc;
  const void* A;
  const void* B;
  const void* draw;
  int64_t ld_draw;
  void* A_new;
  void* zero;
  int64_t zero_bytes;
  int32_t d_in, d_out, r, r_new, draw_cols;
  float scale, acc_beta;
  void* workspace;
  size_t workspace_bytes;
} sow_accumulate_args;
int sow_accumulate_batch(const sow_accumulate_args* items, int n, int dtype, void* stream);

/* Multi-tensor zero fill -- replaces the per-parameter torch.zeros_like of reset_optimizer
 * (scripts/utils/training_utils.py:257-277) and B <- 0 of sow.py:159.  ptrs/bytes are HOST arrays. */
int sow_zero_state(void* const* ptrs, const int64_t* bytes, int n, void* stream);

/* AdamW step over one flat parameter buffer (the factor param group of simple_train.py:502-506).
 * state_dtype = dtype of exp_avg / exp_avg_sq.  step is the 1-based step count.  The betas are double: 1 - beta and the
 * bias corrections are formed from them in double, as torch.optim.AdamW does, and rounded to fp32 once. */
int sow_adamw_flat(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, int64_t n, float lr, double beta1,
                   double beta2, float eps, float weight_decay, int step, float grad_scale, int dtype, int state_dtype,
                   void* stream);

/* AdamW over segments of one flat buffer: every segment [begin, end) (elements of the flat buffers) steps with its own lr,
 * weight_decay and 1-based step count -- the factors and the biases of a biased model share one FactorBucket but not one
 * torch param group (run_glue.py:796-808), and reset_optimizer zeroes the step of the factor group only.  `segs` is a
 * HOST array, sorted by begin, ranges disjoint and non-empty; elements outside every segment are left untouched in all
 * four buffers.  One launch per SOW_ADAMW_MAX_SEGMENTS segments.  Per segment 1 - lr*wd, lr/bc1 and sqrt(bc2) are formed in double and rounded
 * once, as sow_adamw_flat forms them; the per-element arithmetic is sow_adamw_flat's, so one segment [0, n) reproduces it
 * bit for bit.  Same dtype pairs as sow_adamw_flat.  SOW_ERR_SHAPE: an empty, negative, unsorted or overlapping range, a
 * step < 1, n_segs < 0 (checked for every segment before anything is launched); SOW_ERR_NULL: a null pointer. */
#define SOW_ADAMW_MAX_SEGMENTS 64 /* segments per launch; a longer table takes ceil(n_segs / 64) launches */
typedef struct sow_adamw_segment {
  int64_t begin, end;
  float lr, weight_decay;
  int step;
} sow_adamw_segment;
int sow_adamw_flat_seg(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, const sow_adamw_segment* segs,
                       int n_segs, double beta1, double beta2, float eps, float grad_scale, int dtype, int state_dtype,
                       void* stream);

/* Global gradient statistics of one flat buffer, kept on the device: the norm that torch.nn.utils.clip_grad_norm_ takes
 * (simple_train.py:631, the Trainer's max_grad_norm), the clip coefficient, the one factor AdamW multiplies the gradient by
 * and a flag for gradients that are not finite (the overflow check of an fp16 loop).  The host never reads any of it.
 *   sow_grad_stats_flat   two launches on `stream`: one double per workgroup (at most 1024, each over a range of elements
 *                         that depends on n only; 16-byte loads when grad is 16-byte aligned, element loads of the same
 *                         elements otherwise; every element widened to double, squared and summed in double in a fixed
 *                         order), then one workgroup that sums them in a fixed order and writes the record.  No atomics:
 *                         the bits of the record depend on n, the dtype, the data and the scalars only.  Neither the
 *                         workspace nor `out` has to be initialised.  extra_sumsq, loss_scale, extra_found_inf: DEVICE
 *                         scalars, each may be NULL (0, 1, 0).  skip_counters: n_counters DEVICE int32, each raised by the
 *                         record's nonfinite flag (NULL / 0: none).  n == 0: sumsq = 0 (grad may be NULL).
 *   SOW_ERR_SHAPE: n < 0 or n_counters < 0; SOW_ERR_NULL: out, workspace, grad (n > 0) or skip_counters (n_counters > 0);
 *   SOW_ERR_DTYPE: not SOW_DTYPE_F32 / BF16 / F16; SOW_ERR_WORKSPACE: below sow_grad_stats_workspace_bytes(n) (a pure,
 *   monotone function of n, at most 8 KiB).  All of it before the first launch: a refused call writes nothing. */
typedef struct sow_grad_stats {
  double sumsq;      /* sum of g^2 over the flat buffer as stored (before any scale) */
  double total_sq;   /* mult0^2 * sumsq + extra_sumsq, mult0 = grad_scale / loss_scale */
  float total_norm;  /* (float)sqrt(total_sq) */
  float clip_coef;   /* min(1, max_norm / (sqrt(total_sq) + 1e-6)); exactly 1.0f when max_norm <= 0 or +inf */
  float grad_mult;   /* (float)(mult0 * clip_coef): the one factor AdamW multiplies g by */
  int32_t nonfinite; /* 1 when total_sq is not finite or *extra_found_inf != 0, else 0 */
} sow_grad_stats;
size_t sow_grad_stats_workspace_bytes(int64_t n);
int sow_grad_stats_flat(const void* grad, int64_t n, int dtype, float grad_scale, float max_norm, const double* extra_sumsq,
                        const float* loss_scale, const float* extra_found_inf, int32_t* skip_counters, int n_counters,
                        void* workspace, size_t workspace_bytes, sow_grad_stats* out, void* stream);

/* sow_adamw_flat_seg with the gradient multiplier read from a device record: g is multiplied by stats->grad_mult, and with
 * skip_nonfinite != 0 a record whose nonfinite flag is set leaves param, exp_avg and exp_avg_sq untouched.  `stats` must
 * have been written on `stream` before this call (sow_grad_stats_flat).  seg_counter (HOST, n_segs entries, or NULL for
 * none): per segment an index into the DEVICE array skip_counters, -1 for none.  A segment without a counter, or whose
 * counter reads 0, runs with the host-formed scalars of sow_adamw_flat_seg -- with grad_mult equal to its grad_scale the
 * results are its results bit for bit.  A counter that reads c > 0 makes the kernel form 1 - lr*wd, lr/bc1 and sqrt(bc2)
 * for step max(1, step - c) in double on the device, each rounded once: host step counts advance on skipped steps, the
 * bias correction does not.  Errors as sow_adamw_flat_seg, plus SOW_ERR_NULL for stats (or skip_counters with
 * n_counters > 0) and SOW_ERR_SHAPE for n_counters < 0 or a seg_counter entry outside [-1, n_counters); all before the
 * first launch. */
int sow_adamw_flat_seg_stats(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, const sow_adamw_segment* segs,
                             const int* seg_counter, int n_segs, double beta1, double beta2, float eps,
                             const sow_grad_stats* stats, int skip_nonfinite, const int32_t* skip_counters, int n_counters,
                             int dtype, int state_dtype, void* stream);

/* TTAdam dense section (ttadam.py:84-111), fp32 buffers; double betas (1 - beta formed in double). */
int sow_ttadam_dense(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, double beta1,
                     double beta2, float eps, float step_size, float lr_times_wd, int clamp_v, void* stream);

/* TT Hadamard product of two cores (tt.py:469-475): out[(a,c),ij,(b,d)] = A[a,ij,b] * B[c,ij,d], fp32. */
int sow_tt_kron_core(const float* A, const float* B, float* out, int ra0, int rb0, int ij, int ra1, int rb1,
                     void* stream);

/* Tensor-train optimizer state on device, batched over trains.  A train is described by its fp32 cores
 * (core k: [ranks[k], in_dims[k], out_dims[k], ranks[k+1]], contiguous, ranks[0] = ranks[order] = 1) and the shape
 * [rows, cols] of the matrix it represents (rows <= prod(in_dims), cols <= prod(out_dims): TensorTrain.from_matrix pads,
 * to_matrix un-pads -- tt.py:48-67, 242-247, utils.py:78-87).  ranks <= 32, order <= SOW_TT_MAX_ORDER, ranks[k+1] <=
 * ranks[k] * in_dims[k] * out_dims[k]; anything else returns SOW_ERR_UNSUPPORTED (the caller keeps the per-train path).
 *   sow_tt_reconstruct_batch  out_i[rows, cols] = TensorTrain.to_matrix (tt.py:213-247), one launch per 16 trains;
 *   sow_tt_decompose_batch    cores_i <- TensorTrain.from_matrix(mat_i, ranks, padding=True) (tt.py:48-67 + decompose
 *                             :111-140: sequential truncated complete-mode QR, LAPACK sign convention): per bond ONE
 *                             Householder-panel launch for all trains; workspace per train:
 *                             sow_tt_decompose_workspace_bytes;
 *   sow_ttadam_batch          TTAdam.step (ttadam.py:68-115) for n parameters: reconstruct m and v, clamp v < 0, Adam
 *                             update of the parameter (+ the decoupled weight-decay line :110-111), re-decompose both
 *                             moments into the cores given (in place over the old ones); has_state = 0 on the first step
 *                             (m = v = 0).  step_size already carries the bias correction of :95-100.  The betas are
 *                             double: 1 - beta is formed in double and rounded to fp32 once, as sow_ttadam_dense
 *                             does.  Workspace per item: sow_ttadam_workspace_bytes(&item.m). */
#define SOW_TT_MAX_ORDER 6
typedef struct sow_tt_desc {
  void* cores[SOW_TT_MAX_ORDER];
  int32_t order;
  int32_t ranks[SOW_TT_MAX_ORDER + 1];
  int32_t in_dims[SOW_TT_MAX_ORDER];
  int32_t out_dims[SOW_TT_MAX_ORDER];
  int32_t rows, cols;
} sow_tt_desc;
typedef struct sow_ttadam_item {
  sow_tt_desc m, v;        /* exp_avg / exp_avg_sq trains (read when has_state, always written) */
  float* param;            /* [rows, cols] fp32, row pitch ld_param */
  const float* grad;
  int64_t ld_param, ld_grad;
  float step_size, lr_times_wd;
  int32_t has_state;
  void* workspace;
  size_t workspace_bytes;
} sow_ttadam_item;
size_t sow_tt_decompose_workspace_bytes(const sow_tt_desc* tt);
size_t sow_ttadam_workspace_bytes(const sow_tt_desc* tt);
int sow_tt_reconstruct_batch(const sow_tt_desc* tts, void* const* out, const int64_t* ld_out, int n, void* stream);
int sow_tt_decompose_batch(const sow_tt_desc* tts, const void* const* mats, const int64_t* ld, int n, void* const* workspaces,
                           const size_t* workspace_bytes, void* stream);
int sow_ttadam_batch(const sow_ttadam_item* items, int n, double beta1, double beta2, float eps, void* stream);

/* out[0] = max |x[i]| over n fp32 elements (TensorTrain.sqrt / sqrtinv scaling, tt.py:288, 322).  NaN elements are
 * skipped (fmaxf): the result is the max over the others (0 when all are NaN), where torch.amax would return NaN. */
int sow_absmax(const float* x, int64_t n, float* out, void* stream);

/* Batched inverse of `batch` small [r, r] fp32 matrices, r <= 16 (TensorTrain.reciprocal, tt.py:480-494). */
int sow_small_inverse(const float* A, float* out, int batch, int r, void* stream);

/* y = a*x + b*y over n elements. */
int sow_axpby(const void* x, void* y, int64_t n, float a, float b, int dtype, void* stream);

/* Strided 2-D cast copy between any two of f32 / bf16 / f16 (RNE when narrowing; contiguous 16-byte-aligned buffers take a
 * vectorised kernel).  Casts the fp32 x of a layer under autocast to the compute dtype, and its bf16 / f16 gradient back. */
int sow_cast_copy(const void* src, int64_t lds, int src_dtype, void* dst, int64_t ldd, int dst_dtype, int64_t rows,
                  int cols, void* stream);

/* The image of a SOW_ACC_DENSE_FP8 accumulator:  dst[k, n] = e4m3(q[k, n]) * 2^exps[n]  in SOW_DTYPE_BF16 or SOW_DTYPE_F16,
 * exact (a NaN code gives NaN).  q [d_in, d_out] codes, exps [d_out] int8, dst [d_in, ldd >= d_out]; columns past d_out of a
 * dst row are not written.  One streaming pass: every code read once, 16-byte stores.  d_out and ldd multiples of 8
 * (SOW_ERR_UNSUPPORTED), q and exps 8-byte and dst 16-byte aligned (SOW_ERR_ALIGN), |exps[n]| <= 119. */
int sow_acc_dequantize(const void* q, const void* exps, int d_in, int d_out, void* dst, int64_t ldd, int dst_dtype,
                       void* stream);

/* The image of a SOW_ACC_DENSE_FP4 accumulator:  dst[k, n] = e2m1(code(k, n)) * 2^(scales[k / 32, n] - 127)  in SOW_DTYPE_BF16 or
 * SOW_DTYPE_F16, exact, -0 kept.  codes [d_in / 2, d_out], scales [d_in / 32, d_out] (SOW_ACC_DENSE_FP4 above), dst [d_in,
 * ldd >= d_out]; columns past d_out of a dst row are not written.  One streaming pass: every code read once, 16-byte stores.
 * d_in a multiple of 32, d_out and ldd multiples of 8 (SOW_ERR_UNSUPPORTED), codes and scales 8-byte and dst 16-byte aligned
 * (SOW_ERR_ALIGN).  Error codes as sow_acc_dequantize. */
int sow_acc_dequantize_fp4(const void* codes, const void* scales, int d_in, int d_out, void* dst, int64_t ldd, int dst_dtype,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SOW_AMD_H */
