/*
 * lt_string_expect_long.h -- the alignment expectation and the string scatter
 * of lt_string_expect.h for long label strings, part of the C ABI of
 * liblt_lattice.so. lt_string_expect.h includes this header (and this one
 * includes it), so either include gives all five entry points and
 * include/lt_lattice.h the whole ABI.
 */
#ifndef LT_STRING_EXPECT_LONG_H_
#define LT_STRING_EXPECT_LONG_H_

#include "lt_string_expect.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lt_table_align_expectation for 256 <= max_labels <= 1023. expected,
 * log_prob, emission, blank_occ, cov_lex and cov_blank are exactly what
 * lt_string_expect.h defines, with every rule of its "Fixed behaviour" list (a
 * -inf arc is selected out and its value never multiplied; exact zeros in rows
 * t >= num_frames and columns past num_labels; an unaligned utterance gives
 * log_prob = -inf, expected = 0 and all-zero arrays, never NaN; num_frames = 0
 * with num_labels = 0 gives (0, 0)); the arguments, the NULL rules of the four
 * arrays and the error codes are lt_table_align_expectation's. All four arrays
 * NULL is a value-only call: no history is kept, the workspace may be NULL and
 * the kernel ends where its halves meet. ONE kernel on `stream` (capturable; no
 * allocation, synchronisation or stream of its own), no atomics: two calls
 * give bit-equal outputs; every output element and every workspace byte the
 * kernel reads is written by the call. The per-position arithmetic is
 * lt_table_align_expectation's; the two kernels' ranges do not overlap and
 * their results are not bit-comparable.
 *   One workgroup per utterance: two directions ((alpha, abar) upward, (beta,
 *         bbar) downward, meeting at m = nf / 2) of NW = ceil((U+1)/256) waves
 *         each, 128 NW threads; wave w of a direction holds string positions
 *         256w .. 256w+255. Neighbouring waves hand the recursion's carry --
 *         a triple: integer part, fraction and the conditional mean -- on
 *         through LDS, a block of 16 frames at a time, one workgroup barrier
 *         per block.
 *   workspace: the per-frame history, 12 bytes per frame and position
 *         (integer part and fraction of alpha or beta, and the mean) over
 *         256 NW positions:
 *             batch * max_frames * 256 * NW * 12 bytes, rounded up to 256
 *         (lt_table_align_expectation_long_workspace_bytes(); 8-byte aligned;
 *         0 when batch or max_frames is 0). It is needed only when one of the
 *         four arrays is requested: a value-only call may pass NULL. 0.79 GB
 *         at batch = 64, max_frames = 1000, NW = 4.
 *   LDS rule: 36 bytes per position over 256 NW positions (three position
 *         arrays of 4 bytes, the two midpoint triples of 12: 36 KiB at NW = 4),
 *         then max(staged table bytes, carry ring bytes) rounded up to 16. The
 *         next-state table (4 * num_states * vocab_size bytes) is staged while
 *         it is at most 32 KiB, else it is read from memory and counts 0; the
 *         carry ring, 2 * (NW-1) * 2 * 16 entries of 16 bytes (3 KiB at
 *         NW = 4), takes the table's place after the prologue.
 * Range: FrameDependent (expansions == 0), 256 <= max_labels <= 1023, fewer
 * than 2^31 weights per frame, fp32 or bf16 weights, any max_frames, any
 * next-state table; outside it -- max_labels <= 255, lt_table_align_expectation's
 * range, included -- LT_EUNSUPPORTED from the query on and nothing is launched.
 * in_offsets / in_arcs of *g are not read. */
int lt_table_align_expectation_long_workspace_bytes(const lt_graph* g, const lt_table_problem* pb,
                                                    size_t* bytes);
int lt_table_align_expectation_long(const lt_graph* g, const lt_table_problem* pb, const void* W,
                                    const float* lexical_values /* [B,T,U] */,
                                    const float* blank_values /* [B,T,U+1] */,
                                    const int32_t* num_frames, const int32_t* labels,
                                    const int32_t* num_labels, float* expected /* [B] */,
                                    float* log_prob /* [B] */,
                                    float* emission /* [B,T,U], nullable */,
                                    float* blank_occ /* [B,T,U+1], nullable */,
                                    float* cov_lex /* [B,T,U], nullable */,
                                    float* cov_blank /* [B,T,U+1], nullable */, void* workspace,
                                    size_t workspace_bytes, void* stream);

/* lt_table_string_scatter for 256 <= max_labels <= 1023: the same dW, the same
 * summation rule (string arcs that share a cell are summed by the first of
 * them in ascending position order, the blank arc of a position before its
 * lexical arc; one writer per element and frame, no atomics, two calls give
 * bit-equal outputs), every element of dW written by ONE capturable kernel in
 * which a workgroup owns 64 rows of one utterance, zeroes them and, behind a
 * workgroup barrier, writes the sums. The arcs that share a cell are found by
 * sorting the 2 (max_labels + 1) string entries by (cell, entry) in LDS, not by
 * comparing all pairs. pb->weight_dtype is not read.
 * Range: as lt_table_align_expectation_long, else LT_EUNSUPPORTED. */
int lt_table_string_scatter_long(const lt_graph* g, const lt_table_problem* pb,
                                 const float* g_lex /* [B,T,U] */,
                                 const float* g_blank /* [B,T,U+1] */, const int32_t* num_frames,
                                 const int32_t* labels, const int32_t* num_labels,
                                 float* dW /* [B,T,C,V+1] */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LT_STRING_EXPECT_LONG_H_ */
