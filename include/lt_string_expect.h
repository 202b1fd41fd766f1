/*
 * lt_string_expect.h -- expected values over the alignments of a label string
 * with their gradients, and the scatter from string coordinates to the dense
 * arc-weight gradient; part of the C ABI of liblt_lattice.so.
 * include/lt_lattice.h includes this header (and this one includes it, for
 * lt_graph / lt_table_problem and the conventions: device pointers, stream
 * ordering, LT_E* return codes), so either include gives the whole ABI.
 */
#ifndef LT_STRING_EXPECT_H_
#define LT_STRING_EXPECT_H_

#include "lt_lattice.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The expectation of an arc-additive path value under the posterior over the
 * alignments of one transcript. The lattice is the string lattice of
 * lt_posterior.h: positions u = 0..nl, blank_t[u] = W[t, ctx_u, 0], lex_t[u] =
 * W[t, ctx_u, y_{u+1}], alpha, beta and log_prob as defined there; labels
 * outside 1..V are epsilons, as there. A path pi takes one arc per live frame
 * t < nf. Values are given in string coordinates:
 *   lexical_values[t, u]  [B, T, U]    the arc leaving position u on frame t
 *   blank_values[t, u]    [B, T, U+1]  the blank arc at position u on frame t
 *
 *   p(pi)          = exp(w(pi) - log_prob),   v(pi) = sum_{a in pi} v_a
 *   expected       = sum_pi p(pi) v(pi)
 *                  = sum_{t,u} emission[t,u] lexical_values[t,u]
 *                  + sum_{t,u} blank_occ[t,u] blank_values[t,u]
 *   emission[t,u]  = exp(alpha_t[u] + lex_t[u]   + beta_{t+1}[u+1] - log_prob)
 *                  = d log_prob / d lex_t[u]   = d expected / d lexical_values[t,u]
 *   blank_occ[t,u] = exp(alpha_t[u] + blank_t[u] + beta_{t+1}[u]   - log_prob)
 *                  = d log_prob / d blank_t[u] = d expected / d blank_values[t,u]
 *
 * Two fp32 vectors travel beside alpha and beta in conditional-mean form
 * (never the log of a sum of values, so values may have any sign): abar_t[u],
 * the posterior mean of the prefix value given position u before frame t, and
 * bbar_t[u], the mean of the suffix value from position u.
 *   abar_{t+1}[u] = the softmax-weighted mean of abar_t[u] + bv_t[u] and
 *                   abar_t[u-1] + lv_t[u-1], with weights
 *                   exp(alpha_t[u] + blank_t[u] - alpha_{t+1}[u]) and
 *                   exp(alpha_t[u-1] + lex_t[u-1] - alpha_{t+1}[u])
 *   bbar_t[u]     = the same over the two out-arcs of u
 *   E[v | lexical arc (t,u)] = abar_t[u] + lv_t[u] + bbar_{t+1}[u+1]
 *   E[v | blank arc (t,u)]   = abar_t[u] + bv_t[u] + bbar_{t+1}[u]
 *   cov_lex[t,u]   = emission[t,u]  (E[v | lexical arc] - expected) = d expected / d lex_t[u]
 *   cov_blank[t,u] = blank_occ[t,u] (E[v | blank arc]   - expected) = d expected / d blank_t[u]
 *   expected       = sum_u exp(alpha_m[u] + beta_m[u] - log_prob) (abar_m[u] + bbar_m[u])
 * for any frame m; the kernel takes m = nf / 2, where its two halves meet, and
 * log_prob = logsumexp_u(alpha_m[u] + beta_m[u]) there, as lt_posterior.h.
 *
 * Fixed behaviour.
 *   - An arc of weight -inf has emission = blank_occ = cov = 0 and its value is
 *     never multiplied into anything: NaN or inf there is harmless.
 *   - A position with alpha = -inf has abar = 0 (beta, bbar likewise).
 *   - Rows t >= nf of the four arrays are exactly 0 and the values there are not
 *     read; likewise columns u >= nl of the lexical arrays and u > nl of the
 *     blank arrays.
 *   - log_prob not finite (no path, -inf arcs on every path, num_labels outside
 *     [0, U]): log_prob = -inf, expected = 0, the four arrays all zero; never NaN.
 *   - nf = 0 with nl = 0: expected = 0, log_prob = 0.
 *
 *   W [B,T,C,V+1] fp32 or bf16 (pb->weight_dtype; bf16 widened exactly); values,
 *   expected [B], log_prob [B] and the four arrays fp32.
 *   emission, cov_lex [B,T,U]; blank_occ, cov_blank [B,T,U+1]: each may be NULL;
 *   every element of a non-NULL array is written; they carry no
 *   incoming-gradient factor. All four NULL is a value-only call: no history is
 *   kept (the workspace may be NULL) and the kernel ends where its halves meet.
 * ONE kernel on `stream` (capturable; no allocation, synchronisation or stream
 * of its own), one 128-thread workgroup per utterance, no atomics: two calls
 * give bit-equal outputs.
 * Range: FrameDependent (expansions == 0), max_labels <= 255, fewer than 2^31
 * weights per frame, fp32 or bf16 weights, any max_frames, any next-state
 * table; outside it LT_EUNSUPPORTED, also from the workspace query, and nothing
 * is launched.
 * LDS rule: the history holds 12 bytes per frame and position (integer part
 * and fraction of alpha or beta, and the mean). With SP = 64 * ceil((U+1)/64)
 * rounded up to 64, 128 or 256 positions it stays in LDS while
 *   36 * SP + max(12 * SP * max_frames, staged table bytes) <= 160 KiB
 * (36 * SP: three position arrays and the two midpoint triples; the
 * next-state table is staged while it is at most 32 KiB and shares the
 * history's space), i.e. max_frames <= 210 at SP = 64, 103 at SP = 128, 50 at
 * SP = 256 with a table of at most 32 KiB. Else it is in `workspace`:
 * lt_table_align_expectation_workspace_bytes() bytes, 8-byte aligned (0 when
 * unused; then it may be NULL). in_offsets / in_arcs of *g are not read. */
int lt_table_align_expectation_workspace_bytes(const lt_graph* g, const lt_table_problem* pb,
                                               size_t* bytes);
int lt_table_align_expectation(const lt_graph* g, const lt_table_problem* pb, const void* W,
                               const float* lexical_values /* [B,T,U] */,
                               const float* blank_values /* [B,T,U+1] */,
                               const int32_t* num_frames, const int32_t* labels,
                               const int32_t* num_labels, float* expected /* [B] */,
                               float* log_prob /* [B] */, float* emission /* [B,T,U], nullable */,
                               float* blank_occ /* [B,T,U+1], nullable */,
                               float* cov_lex /* [B,T,U], nullable */,
                               float* cov_blank /* [B,T,U+1], nullable */, void* workspace,
                               size_t workspace_bytes, void* stream);

/* The scatter from string coordinates to the dense arc-weight gradient: for
 * every live frame t < num_frames[b] (clamped to [0, T]) and with nl =
 * num_labels[b] clamped to [0, U],
 *   dW[t, ctx_u, y_{u+1}] += g_lex[t, u]    for u <  nl
 *   dW[t, ctx_u, 0]       += g_blank[t, u]  for u <= nl
 * and every other element of dW [B,T,C,V+1] (fp32) is 0. Rows t >= num_frames
 * and columns past nl of g_lex [B,T,U] / g_blank [B,T,U+1] are not read. An
 * epsilon label reads label 1's weight, so its lexical gradient lands on
 * label 1's cell of its context state (what autograd through the gather does).
 * String arcs that share a cell (a repeated bigram: "abab") are summed by the
 * first of them in ascending position order, the blank arc of a position
 * before its lexical arc: one writer per element and frame, no atomics, two
 * calls give bit-equal outputs. Every element of dW is written: ONE kernel on
 * `stream` (capturable; no memset, allocation, synchronisation or stream of
 * its own) in which a workgroup owns 64 rows of one utterance, zeroes them and,
 * behind a workgroup barrier, writes the sums. pb->weight_dtype is not read.
 * Range: as lt_table_align_expectation, else LT_EUNSUPPORTED. */
int lt_table_string_scatter(const lt_graph* g, const lt_table_problem* pb,
                            const float* g_lex /* [B,T,U] */,
                            const float* g_blank /* [B,T,U+1] */, const int32_t* num_frames,
                            const int32_t* labels, const int32_t* num_labels,
                            float* dW /* [B,T,C,V+1] */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LT_STRING_EXPECT_H_ */
