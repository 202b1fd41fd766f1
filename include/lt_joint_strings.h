/*
 * lt_joint_strings.h -- the rows of the joint weight function's arc weights
 * that a label string visits, formed without W [B,T,C,V+1]: what forced
 * alignment (lt_table_align, lt_table_align_long) and the emission posteriors
 * (lt_table_align_posteriors, lt_table_align_posteriors_long) of a
 * large-context joint model read. Part of the C ABI of liblt_lattice.so;
 * include/lt_lattice.h includes this header (and this one includes it, for
 * lt_graph / lt_table_problem / lt_joint_params and the conventions), so either
 * include gives the whole ABI.
 */
#ifndef LT_JOINT_STRINGS_H_
#define LT_JOINT_STRINGS_H_

#include "lt_lattice.h"

#ifdef __cplusplus
extern "C" {
#endif

/* With s_k(b) the context state of g's table after the first k non-epsilon
 * labels of utterance b's U = pb->max_labels label slots (a label outside 1..V
 * is an epsilon; all U slots count, whatever num_labels holds, as the string
 * kernels' prologue walks them) and n_b the number of those labels,
 *   Ws[b,t,k,y] = out_bias[y] + sum_h out_weight[y,h] tanh(ctx_proj[s_k(b),h] + frame_proj[b*T+t,h])
 * for 0 <= k <= n_b and t < num_frames[b] (clamped to [0, T]), 0 elsewhere.
 *
 * The chain table. On the table of U+1 states with next[k, y-1] = min(k+1, U)
 * for every label y, a string kernel is in state k after k non-epsilon labels.
 * So on (that table, Ws, the same labels) it reads, element for element and in
 * the same order, what it reads on (g, W = lt_joint_weights_ex's output), and
 * returns the same bits -- at B T (U+1) (V+1) values instead of B T C (V+1)
 * (a 4-gram over 32 labels at B = 64, T = 1000, U = 100: 0.85 GB for 286 GB).
 *
 * Bit identity. While every |ctx_proj| of a visited row and every |frame_proj|
 * is <= 40, each live element equals lt_joint_weights_ex's W[b,t,s_k,y] bit for
 * bit, in the same precision (LT_JOINT_SPLIT / LT_JOINT_BF16) and the same
 * output dtype: tanh from e^{2a} e^{2b}, 32 x 32 tiles of
 * v_mfma_f32_32x32x16_bf16 over the hidden units h = 0, 16, ... in the
 * producer's order, the bias added and the result rounded as the producer does
 * it. Past 40 (or NaN) both fall back to tanh from e^{2(a+b)}, but not over the
 * same ranges: here a visited ctx_proj row over 40 switches its utterance and a
 * frame_proj row over 40 its frame, while the producer switches per block of 32
 * frames or globally. Then only the producer's accuracy holds (split products:
 * about 16 mantissa bits each, fp32 sums), not bit identity.
 *
 *   g            the model's graph; only next_state is read. expansions = 0.
 *   pb           batch B, max_frames T, max_labels U; weight_dtype is the dtype
 *                of Ws, LT_DTYPE_F32 or LT_DTYPE_BF16, as in lt_joint_weights_ex.
 *   jp           hidden, precision, ctx_proj [C, hidden], frame_proj
 *                [B*T, hidden], out_weight [V+1, hidden], out_bias [V+1];
 *                the projections 16-byte aligned.
 *   num_labels   [B] or NULL; not read (the rows cover all U slots).
 *   Ws           [B,T,U+1,V+1]; may exceed 2^31 elements (offsets are 64-bit).
 *   states       [B,U+1] or NULL: s_k for k <= n_b, -1 past n_b.
 *   workspace    lt_joint_string_rows_workspace_bytes() bytes, 16-byte aligned:
 *                per utterance the over-40 flag and n_b, s_k [B,U+1], and the
 *                gathered rows e^{2 ctx_proj[s_k]} [B,U+1,hidden] fp32
 *                (ctx_proj[s_k] itself for an utterance over 40).
 * Two launches on `stream` (capturable; no allocation, synchronisation, memset
 * or stream of their own): the walk and gather, one workgroup per utterance,
 * then the row producer, one workgroup per (utterance, 32 chain rows, frame
 * slice). Every element of Ws and states is written by the call
 * (zeros for padding frames and dead rows, -1 for states past n_b), and every
 * workspace byte read is written first; reruns are bit-equal.
 * LT_EINVAL: a NULL g, pb, jp, num_frames, labels, workspace or projection
 * pointer (Ws and frame_proj may be NULL when T = 0), a bad graph or negative
 * shape, hidden < 1, a precision other than LT_JOINT_SPLIT / LT_JOINT_BF16, a
 * weight_dtype other than fp32 / bf16, a misaligned pointer, a workspace that
 * is too small. LT_EUNSUPPORTED, nothing launched: expansions >= 1, V + 1 > 64,
 * hidden no multiple of 16 or above 1024, max_labels outside [1, 4095], or an
 * LDS image above the CU's 160 KB: out_weight as bf16 hi (+ lo for split
 * products) in rows of hidden + 8 and four frame rows of hidden fp32, i.e.
 * (4 or 2) (V+1) (hidden + 8) + 16 hidden bytes. V + 1 = 33 fits at every
 * hidden; V + 1 = 64 fits up to hidden = 592 with split products and at every
 * hidden with bf16 products. */
int lt_joint_string_rows_workspace_bytes(const lt_graph* g, const lt_table_problem* pb,
                                         const lt_joint_params* jp, size_t* bytes);
int lt_joint_string_rows(const lt_graph* g, const lt_table_problem* pb, const lt_joint_params* jp,
                         const int32_t* num_frames, const int32_t* labels /* [B,U] */,
                         const int32_t* num_labels,
                         void* Ws /* [B,T,U+1,V+1], pb->weight_dtype */,
                         int32_t* states /* [B,U+1], nullable: s_k, -1 past n_b */,
                         void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LT_JOINT_STRINGS_H_ */
