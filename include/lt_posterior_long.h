/*
 * lt_posterior_long.h -- the emission posteriors of lt_posterior.h for long
 * label strings, part of the C ABI of liblt_lattice.so. lt_posterior.h
 * includes this header (and this one includes it), so either include gives
 * both entry points and include/lt_lattice.h the whole ABI.
 */
#ifndef LT_POSTERIOR_LONG_H_
#define LT_POSTERIOR_LONG_H_

#include "lt_posterior.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lt_table_align_posteriors for 256 <= max_labels <= 1023. emission and
 * log_prob are exactly what lt_posterior.h defines (epsilons, exact zeros in
 * rows t >= num_frames and columns u >= num_labels, log_prob = -inf with an
 * all-zero emission for an unaligned utterance, never NaN, num_frames = 0
 * with num_labels = 0: log_prob = 0); the arguments, alignment rules, NULL
 * rules and error codes are lt_table_align_posteriors'. ONE kernel on
 * `stream` (capturable; no allocation, synchronisation or stream of its own),
 * no atomics (a call is deterministic), every output element and every
 * workspace byte the kernel reads is written by the call.
 *   One workgroup per utterance: two directions (alpha upward, beta
 *         downward, meeting at m = nf / 2) of NW = ceil((U+1)/256) waves each,
 *         128 NW threads; wave w of a direction holds string positions
 *         256w .. 256w+255. Neighbouring waves hand the recursion's carry on
 *         through LDS, a block of 16 frames at a time, one workgroup barrier
 *         per block.
 *   workspace: the per-frame alpha / beta history, 8 bytes per frame and
 *         position over 256 NW positions, always:
 *             batch * max_frames * 256 * NW * 8 bytes, rounded up to 256
 *         (lt_table_align_posteriors_long_workspace_bytes(); 8-byte aligned;
 *         0 only when batch or max_frames is 0, then it may be NULL). 0.52 GB
 *         at batch = 64, max_frames = 1000, NW = 4.
 *   LDS: 28 bytes per position (28 KiB at NW = 4) and the staged next-state
 *         table (at most 32 KiB; the carry ring, 1.5 KiB at NW = 4, takes its
 *         place).
 * Range: FrameDependent (expansions == 0), 256 <= max_labels <= 1023, fewer
 * than 2^31 weights per frame, fp32 or bf16 weights, any max_frames, any
 * next-state table; outside it -- max_labels <= 255, lt_table_align_posteriors'
 * range, included -- LT_EUNSUPPORTED from the query on and nothing is
 * launched. in_offsets / in_arcs of *g are not read. */
int lt_table_align_posteriors_long_workspace_bytes(const lt_graph* g, const lt_table_problem* pb,
                                                   size_t* bytes);
int lt_table_align_posteriors_long(const lt_graph* g, const lt_table_problem* pb, const void* W,
                                   const int32_t* num_frames, const int32_t* labels,
                                   const int32_t* num_labels, float* emission /* [B,T,U] */,
                                   float* log_prob /* [B] */, void* workspace,
                                   size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LT_POSTERIOR_LONG_H_ */
