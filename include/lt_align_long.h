/*
 * lt_align_long.h -- the forced alignment of lt_align.h for long label
 * strings, part of the C ABI of liblt_lattice.so. lt_align.h includes this
 * header (and this one includes it), so either include gives both entry
 * points and include/lt_lattice.h the whole ABI.
 */
#ifndef LT_ALIGN_LONG_H_
#define LT_ALIGN_LONG_H_

#include "lt_align.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lt_table_align for 256 <= max_labels <= 4095. The definition, the tie
 * rules, the epsilon handling, the three outputs' layout and the
 * unaligned-utterance rule are lt_table_align's (lt_align.h), and so are the
 * arguments, the NULL and alignment rules and the error codes and messages.
 * ONE kernel on `stream` (capturable; no allocation, synchronisation or stream
 * of its own), no atomics (a call is deterministic), every output element and
 * every workspace byte the kernel reads is written by the call.
 *   One workgroup per utterance of NW = ceil((max_labels+1)/256) waves (2 ..
 *         16, 64 NW threads); wave w holds string positions 256w .. 256w+255,
 *         four consecutive ones a lane. Neighbouring waves hand the
 *         recursion's carry on through LDS, a block of 16 frames at a time,
 *         one workgroup barrier per block; the waves above an utterance's own
 *         num_labels only pass the barriers.
 *   workspace: the winning terms, one bit per frame and position, always:
 *             word (b, t, w, j), bit l = position 256w + 4l + j of frame t
 *             took its lexical term; [batch, max_frames, NW, 4] 64-bit words,
 *             batch * max_frames * 32 * NW bytes, rounded up to 256
 *         (lt_table_align_long_workspace_bytes(); 8-byte aligned; 0 only when
 *         batch or max_frames is 0, then it may be NULL). 138 MB at batch =
 *         64, max_frames = 4200, NW = 16. The backtrace runs in the same
 *         launch and stages them back through LDS, 256 frames at a time.
 *   LDS: 12 bytes per position (48 KiB at NW = 16) and the staged next-state
 *         table (at most 32 KiB; the carry ring and the backtrace's 16 KiB
 *         staging band take its place).
 * Range: FrameDependent (expansions == 0), 256 <= max_labels <= 4095, fewer
 * than 2^31 weights per frame, fp32 or bf16 weights, any max_frames, any
 * next-state table; outside it -- max_labels <= 255, lt_table_align's range,
 * included -- LT_EUNSUPPORTED from the query on, lt_last_error() set and
 * nothing launched. batch == 0 returns 0 with nothing launched. in_offsets /
 * in_arcs of *g are not read. */
int lt_table_align_long_workspace_bytes(const lt_graph* g, const lt_table_problem* pb,
                                        size_t* bytes);
int lt_table_align_long(const lt_graph* g, const lt_table_problem* pb, const void* W,
                        const int32_t* num_frames, const int32_t* labels,
                        const int32_t* num_labels, int64_t* alignment_labels /* [B, T] */,
                        int64_t* label_frames /* [B,U], nullable */, float* path_weight /* [B] */,
                        void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LT_ALIGN_LONG_H_ */
