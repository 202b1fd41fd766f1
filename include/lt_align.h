/*
 * lt_align.h -- forced alignment of label strings, part of the C ABI of
 * liblt_lattice.so. include/lt_lattice.h includes this header (and this one
 * includes it, for lt_graph / lt_table_problem and the conventions: device
 * pointers, stream ordering, LT_E* return codes), so either include gives
 * the whole ABI.
 */
#ifndef LT_ALIGN_H_
#define LT_ALIGN_H_

#include "lt_lattice.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Forced alignment: the MaxTropical best path of the lattice intersected
 * with the label string (the string acceptor of lt_table_num_forward;
 * RecognitionLattice._string_forward, lattices.py:250-377) -- on which frame
 * each label of the transcript is emitted. Forward and backtrace are ONE
 * kernel on `stream` (capturable; no allocation, synchronisation or stream
 * of its own), one wave per utterance. Any next-state table (FullNGram
 * through its next_state_table()), FrameDependent or FrameLabelDependent(K).
 *   Ties  FrameDependent: the blank term wins when it is >= the lexical one;
 *         FrameLabelDependent: the fewest expansions win; the path is walked
 *         back from position num_labels (as lt_table_num_backward in
 *         LT_SEMIRING_MAX). Sums are fp32 in lt_table_num_forward's order.
 *   labels outside 1..V are epsilons: they read label 1's weight and keep
 *         the context state.
 *   alignment_labels [B, T*A] int64, A = 1 (FrameDependent) or K+1, the slot
 *         layout of lt_table_viterbi: slot i of frame t = the TRUE label y of
 *         the (i+1)-th lexical arc the path takes in that frame (0 for an
 *         epsilon), else 0; the last FrameLabelDependent slot and padding
 *         frames are 0. There is no label_convention (defect D5 is not
 *         reproduced).
 *   label_frames [B, U] int64 (nullable): the frame on which the arc leaving
 *         string position u is taken; -1 for u >= num_labels.
 *   path_weight [B]: bit-equal to lt_table_num_forward(LT_SEMIRING_MAX).
 *   An utterance whose path_weight is not above -inf (no path, -inf arcs,
 *   num_labels outside [0, U]) is unaligned: its alignment_labels row is all
 *   0 and its label_frames row all -1.
 * Range: max_labels <= 255, expansions <= 15, fewer than 2^31 weights per
 * frame; outside it LT_EUNSUPPORTED and nothing is launched. The winning
 * terms (one bit, or ceil(log2(K+1)) bits, per frame and position) stay in
 * LDS while max_frames of them fit 160 KiB, else in `workspace`
 * (lt_table_align_workspace_bytes() bytes, 8-byte aligned; 0 when unused,
 * then it may be NULL). in_offsets / in_arcs of *g are not read. */
int lt_table_align_workspace_bytes(const lt_graph* g, const lt_table_problem* pb, size_t* bytes);
int lt_table_align(const lt_graph* g, const lt_table_problem* pb, const void* W,
                   const int32_t* num_frames, const int32_t* labels, const int32_t* num_labels,
                   int64_t* alignment_labels /* [B, T*A] */, int64_t* label_frames /* [B,U], nullable */,
                   float* path_weight /* [B] */, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LT_ALIGN_H_ */
