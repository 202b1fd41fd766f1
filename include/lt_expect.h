/*
 * lt_expect.h -- posterior means of arc values (expectations under the path
 * posterior, with their gradients), part of the C ABI of liblt_lattice.so.
 * include/lt_lattice.h includes this header (and this one includes it, for
 * lt_graph / lt_table_problem and the conventions: device pointers, stream
 * ordering, LT_E* return codes), so either include gives the whole ABI.
 */
#ifndef LT_EXPECT_H_
#define LT_EXPECT_H_

#include "lt_lattice.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The expectation of an arc-additive path value under the path posterior of
 * the denominator lattice (all label sequences): any next-state table
 * (FullNGram through its next_state_table()) x FrameDependent. Every state is
 * final, a path starts at state 0 and takes one arc per live frame
 * t < num_frames[b] (num_frames is clamped to [0, T]): blank (y = 0, the
 * state stays) or label y (state p -> next_state[p, y-1]).
 *
 * With w_a = W[b,t,p,y] and v_a = values[b,t,p,y] on arc a = (t, p, y),
 *   w(pi) = sum_{a in pi} w_a,  v(pi) = sum_{a in pi} v_a,
 *   p(pi) = exp(w(pi)) / Z_b,   log_z[b] = log Z_b,
 *   expected[b] = E_b = sum_pi p(pi) v(pi) = sum_a m_a v_a,
 *   marg[a] = dE_b / dv_a = d log Z_b / dw_a = m_a, the arc marginal (what
 *             lt_table_den_backward writes in LT_SEMIRING_LOG),
 *   cov[a]  = dE_b / dw_a = m_a (E[v(pi) | a in pi] - E_b), the covariance of
 *             the arc indicator with the path value.
 *
 * Recurrences. Beside alpha_t(q) (the Log forward vector: state q before
 * frame t) travels abar_t(q), the posterior mean of the prefix value given
 * that the path is in q before frame t; beside beta_{t+1}(q') travels
 * bbar_{t+1}(q'), the mean of the suffix value from q'.
 *   abar_{t+1}(q) = the softmax-weighted mean of abar_t(p) + v_a over the
 *     in-arcs a: p -> q of frame t, the blank self-arc included, with weights
 *     exp(alpha_t(p) + w_a - alpha_{t+1}(q)); bbar likewise over the out-arcs.
 *   For arc a: p -> q' on frame t:
 *     m_a        = exp(alpha_t(p) + w_a + beta_{t+1}(q') - log Z)
 *     E[v | a]   = abar_t(p) + v_a + bbar_{t+1}(q')
 *   E_b = sum_q exp(alpha_T(q) - log Z) abar_T(q), T = num_frames[b].
 * The means are kept in this conditional-mean form in fp32 (never the log of
 * a sum of values), so values may have any sign.
 *
 * Fixed behaviour.
 *   - An arc with w_a = -inf has marg = cov = 0 and its value is never
 *     multiplied into anything: a NaN or infinite value there is harmless.
 *   - A state with alpha = -inf has abar = 0 (beta, bbar likewise).
 *   - num_frames[b] = 0: expected = 0, log_z = 0, marg = cov = 0.
 *   - log_z[b] not finite: expected = 0, marg = cov = 0, log_z as computed.
 *   - Padding frames t >= num_frames[b] get marg = cov = 0.
 *
 *   W      [B,T,C,V+1] fp32 or bf16 (pb->weight_dtype; bf16 widened exactly)
 *   values [B,T,C,V+1] fp32
 *   expected, log_z [B] fp32
 *   marg, cov [B,T,C,V+1] fp32, either may be NULL. They carry no
 *          incoming-gradient factor. Both NULL is a value-only call: only the
 *          forward kernel is launched and no history is kept.
 *   workspace: lt_table_expectation_workspace_bytes() bytes, the histories of
 *          alpha and abar, [B,T,C] fp32 each (required by every call).
 * Two kernels on `stream` (capturable; no allocation, synchronisation or
 * stream of its own), one workgroup per utterance. No atomics on memory: two
 * calls give bit-equal outputs.
 * expansions >= 1 (FrameLabelDependent): LT_EUNSUPPORTED, also from the
 * workspace query, and nothing is launched. A NULL required pointer, a
 * negative shape, a short workspace or a bad dtype: LT_EINVAL. State vectors
 * past the table kernels' 160 KiB LDS rule, or 2^31 weights or more per
 * frame: LT_EUNSUPPORTED. */
int lt_table_expectation_workspace_bytes(const lt_graph* g, const lt_table_problem* pb,
                                         size_t* bytes);
int lt_table_expectation(const lt_graph* g, const lt_table_problem* pb, const void* W,
                         const float* values /* [B,T,C,V+1] */, const int32_t* num_frames,
                         float* expected /* [B] */, float* log_z /* [B] */,
                         float* marg /* [B,T,C,V+1], nullable */,
                         float* cov /* [B,T,C,V+1], nullable */, void* workspace,
                         size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LT_EXPECT_H_ */
