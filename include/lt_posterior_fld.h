/*
 * lt_posterior_fld.h -- the emission posteriors of lt_posterior.h on the
 * FrameLabelDependent lattice, part of the C ABI of liblt_lattice.so.
 * lt_posterior.h includes this header (and this one includes it), so either
 * include gives every entry point and include/lt_lattice.h the whole ABI.
 */
#ifndef LT_POSTERIOR_FLD_H_
#define LT_POSTERIOR_FLD_H_

#include "lt_posterior.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lt_table_align_posteriors for FrameLabelDependent(K), K = g->expansions >=
 * 1: a frame takes up to K lexical arcs, then the mandatory blank. W is the
 * same [B, T, C, V+1]; the weights do not depend on the expansion slot. With
 * lt_posterior.h's blank_t / lex_t, per utterance, within frame t:
 *   x_0[u] = alpha_t[u]
 *   x_i[u] = x_{i-1}[u-1] + lex_t[u-1]             (i = 1..K; -inf for u < i)
 *   alpha_{t+1}[u] = blank_t[u] + logsumexp_{i=0..K} x_i[u]
 *   y_0[u] = blank_t[u] + beta_{t+1}[u]
 *   y_j[u] = lex_t[u] + y_{j-1}[u+1]               (j = 1..K; no arc out of nl)
 *   beta_t[u] = logsumexp_{j=0..K} y_j[u]
 * alpha_0, beta_nf and log_prob = alpha_nf[nl] as in lt_posterior.h, and
 *   emission[t, u] = sum over i, j >= 0, i + j + 1 <= K of
 *                    exp(x_i[u] + lex_t[u] + y_j[u+1] - log_prob)
 *                  = d log_prob / d lex_t[u]:
 * the posterior probability that the arc leaving string position u is taken
 * on frame t, summed over the frame's expansion slots. Each column u <
 * num_labels of an aligned utterance sums to 1 over the frames; a row sums to
 * at most K. Epsilons, the exact zeros in rows t >= num_frames and columns
 * u >= num_labels, log_prob = -inf with an all-zero emission for an unaligned
 * utterance (never NaN), num_frames = 0 with num_labels = 0: log_prob = 0,
 * the arguments, alignment rules, NULL rules and error codes are
 * lt_table_align_posteriors'. ONE kernel on `stream` (capturable; no
 * allocation, synchronisation or stream of its own), one 128-thread workgroup
 * per utterance, no atomics (a call is deterministic), every output element
 * and every workspace byte the kernel reads is written by the call.
 *   log_prob is evaluated where the two halves meet, as logsumexp_u(alpha_m[u]
 *         + beta_m[u]) at the frame boundary m = nf / 2, and normalises every
 *         frame.
 *   workspace / LDS: lt_table_align_posteriors' rule -- ONE history vector a
 *         frame (8 bytes per frame and position over 64, 128 or 256
 *         positions) whatever K is, in LDS while max_frames rows fit 160 KiB
 *         beside the prologue's arrays, else in `workspace`
 *         (lt_table_align_posteriors_fld_workspace_bytes() bytes, 8-byte
 *         aligned; 0 when unused, then it may be NULL).
 * Range: 1 <= expansions <= 15, max_labels <= 255, fewer than 2^31 weights
 * per frame, fp32 or bf16 weights, any max_frames, any next-state table;
 * outside it -- expansions == 0, lt_table_align_posteriors' range, included
 * -- LT_EUNSUPPORTED from the query on and nothing is launched. in_offsets /
 * in_arcs of *g are not read. */
int lt_table_align_posteriors_fld_workspace_bytes(const lt_graph* g, const lt_table_problem* pb,
                                                  size_t* bytes);
int lt_table_align_posteriors_fld(const lt_graph* g, const lt_table_problem* pb, const void* W,
                                  const int32_t* num_frames, const int32_t* labels,
                                  const int32_t* num_labels, float* emission /* [B,T,U] */,
                                  float* log_prob /* [B] */, void* workspace,
                                  size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LT_POSTERIOR_FLD_H_ */
