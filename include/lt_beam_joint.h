/*
 * lt_beam_joint.h -- prefix beam search with the joint weight function fused
 * in: the arc weights are formed on the matrix cores for the beam's context
 * states only and never written to memory. Part of the C ABI of
 * liblt_lattice.so; include/lt_lattice.h includes this header (and this one
 * includes it, for lt_graph / lt_table_problem / lt_joint_params and the
 * conventions), so either include gives the whole ABI.
 */
#ifndef LT_BEAM_JOINT_H_
#define LT_BEAM_JOINT_H_

#include "lt_lattice.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lt_table_beam_search (include/lt_beam.h: candidates, merge, total order,
 * hashes, trace, outputs, degenerate cases -- all of it) on the fp32 weights
 *   W[b,t,c,y] = out_bias[y] + sum_h out_weight[y,h] tanh(ctx_proj[c,h] + frame_proj[b*T+t,h])
 * formed as lt_joint_weights_ex forms them in jp->precision. A beam of K slots
 * reads K of a frame's C rows, so only those are formed: 32 x 32 tiles of
 * v_mfma_f32_32x32x16_bf16 over the hidden units h = 0, 16, ... in the
 * producer's order, one wave a tile, into LDS, where the search reads them.
 * W [B,T,C,V+1] never exists, so C is bounded by the e^{2 ctx_proj} table
 * [C, hidden] alone (a 4-gram over 32 labels: 69 MB at hidden = 512, where W
 * would be 286 GB at B = 64, T = 1000).
 *
 * Bit identity. While every |ctx_proj| and every |frame_proj| is <= 40, the
 * producer and this kernel both form tanh from e^{2a} e^{2b}, through the same
 * instructions in the same order: labels, num_labels, scores, trace and
 * step_score then equal, bit for bit and in both semirings, what
 * lt_table_beam_search returns on lt_joint_weights_ex's fp32 W. Past 40 both
 * fall back to tanh from e^{2(a+b)}, but not over the same ranges: here a
 * |ctx_proj| > 40 (or NaN) anywhere switches the whole call and a
 * |frame_proj| > 40 switches its own frame, while the producer switches per
 * block of 32 frames or globally. Then only the producer's accuracy holds
 * (split products: about 16 mantissa bits each, fp32 sums), not bit identity.
 *
 *   g, pb        as lt_table_beam_search; pb->weight_dtype is LT_DTYPE_F32
 *                (the dtype of the W that is not written).
 *   jp           hidden, precision, ctx_proj [C, hidden], frame_proj
 *                [B*T, hidden], out_weight [V+1, hidden], out_bias [V+1];
 *                the projections 16-byte aligned.
 *   outputs      as lt_table_beam_search; trace / step_score optional (NULL).
 *   workspace    lt_joint_beam_search_workspace_bytes() bytes, 16-byte
 *                aligned: the |ctx_proj| > 40 flags (1 KiB), e^{2 ctx_proj}
 *                [C, hidden] fp32, then 4*B*T*K bytes of backpointers, which a
 *                call that passes `trace` does not need.
 * Two launches on `stream` (capturable; no allocation, synchronisation, memset
 * or stream of their own): a pre-pass that fills the table and the flags, then
 * the search, one workgroup of 8 waves per utterance. Every
 * output element, and every workspace byte read, is written by the call;
 * reruns are bit-equal.
 * LT_EINVAL: as lt_table_beam_search, a NULL jp or projection pointer, hidden
 * < 1, a precision other than LT_JOINT_SPLIT / LT_JOINT_BF16, a misaligned
 * pointer. LT_EUNSUPPORTED, nothing launched: expansions >= 1, beam_size > 64,
 * V + 1 > 64, hidden no multiple of 16 or above 1024, a weight_dtype other
 * than fp32, 2^31 or more trace elements, or an LDS image (out_weight as bf16
 * hi (+ lo) in rows of hidden + 8, the [64, V+1] weight tile, two frames of
 * the frame ring, the search's rows) above the CU's 160 KB. */
int lt_joint_beam_search_workspace_bytes(const lt_graph* g, const lt_table_problem* pb,
                                         const lt_joint_params* jp, int32_t beam_size,
                                         size_t* bytes);
int lt_joint_beam_search(const lt_graph* g, const lt_table_problem* pb, const lt_joint_params* jp,
                         const int32_t* num_frames, int32_t beam_size, int32_t semiring,
                         int64_t* labels /* [B,K,T] */, int32_t* num_labels /* [B,K] */,
                         float* scores /* [B,K] */, int32_t* trace /* [B,T,K], may be NULL */,
                         float* step_score /* [B,T,K], may be NULL */, void* workspace,
                         size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LT_BEAM_JOINT_H_ */
