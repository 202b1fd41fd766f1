/*
 * lt_posterior.h -- per-label emission posteriors of a label string (soft
 * forced alignment), part of the C ABI of liblt_lattice.so.
 * include/lt_lattice.h includes this header (and this one includes it, for
 * lt_graph / lt_table_problem and the conventions: device pointers, stream
 * ordering, LT_E* return codes), so either include gives the whole ABI.
 */
#ifndef LT_POSTERIOR_H_
#define LT_POSTERIOR_H_

#include "lt_lattice.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Emission posteriors: with what probability is the label at string position
 * u emitted on frame t, given the transcript -- the Log-semiring sibling of
 * lt_table_align. On the lattice intersected with the label string (the
 * string acceptor of lt_table_num_forward), per utterance with nf =
 * num_frames, nl = num_labels, blank_t[u] = W[t, ctx_u, 0] and lex_t[u] =
 * W[t, ctx_u, y_{u+1}] (ctx_u the context state after the first u labels):
 *   alpha_0[u]     = 0 if u == 0 else -inf
 *   alpha_{t+1}[u] = log(exp(alpha_t[u] + blank_t[u]) + exp(alpha_t[u-1] + lex_t[u-1]))
 *   beta_nf[u]     = 0 if u == nl else -inf
 *   beta_t[u]      = log(exp(blank_t[u] + beta_{t+1}[u]) + exp(lex_t[u] + beta_{t+1}[u+1]))
 *   log_prob       = alpha_nf[nl]     (= lt_table_num_forward in LT_SEMIRING_LOG)
 *   emission[t, u] = exp(alpha_t[u] + lex_t[u] + beta_{t+1}[u+1] - log_prob)
 * i.e. the posterior probability that the arc leaving string position u is
 * taken on frame t, = d log_prob / d lex_t[u]. ONE kernel on `stream`
 * (capturable; no allocation, synchronisation or stream of its own), one
 * 128-thread workgroup per utterance, no atomics (a call is deterministic).
 *   labels outside 1..V are epsilons: they read label 1's weight and keep
 *         the context state.
 *   emission [B, T, U] fp32, frame-major. Rows t >= num_frames and columns
 *         u >= num_labels are exactly 0; every element is written. For an
 *         aligned utterance each column u < num_labels sums to 1 over the
 *         frames, and each row sums to at most 1.
 *   log_prob [B] fp32. The kernel evaluates it where its two halves meet, as
 *         logsumexp_u(alpha_m[u] + beta_m[u]) at m = nf / 2 -- the same
 *         number up to fp32 rounding -- and normalises every frame by that
 *         one value.
 *   An utterance whose log_prob is not finite (no path, -inf arcs on every
 *   path, num_labels outside [0, U]) has log_prob = -inf and an all-zero
 *   emission, never NaN. num_frames = 0 with num_labels = 0: log_prob = 0.
 * Range: FrameDependent (expansions == 0), max_labels <= 255, fewer than 2^31
 * weights per frame, fp32 or bf16 weights, any max_frames, any next-state
 * table; outside it LT_EUNSUPPORTED and nothing is launched. The per-frame
 * alpha / beta history (8 bytes per frame and position) stays in LDS while
 * max_frames rows of 64 * ceil((U+1)/64) positions (rounded up to 64, 128 or
 * 256) fit 160 KiB beside the prologue's arrays, else in `workspace`
 * (lt_table_align_posteriors_workspace_bytes() bytes, 8-byte aligned; 0 when
 * unused, then it may be NULL). in_offsets / in_arcs of *g are not read. */
int lt_table_align_posteriors_workspace_bytes(const lt_graph* g, const lt_table_problem* pb,
                                              size_t* bytes);
int lt_table_align_posteriors(const lt_graph* g, const lt_table_problem* pb, const void* W,
                              const int32_t* num_frames, const int32_t* labels,
                              const int32_t* num_labels, float* emission /* [B,T,U] */,
                              float* log_prob /* [B] */, void* workspace, size_t workspace_bytes,
                              void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LT_POSTERIOR_H_ */
