/*
 * lt_beam.h -- prefix beam search: the N best label sequences of the
 * denominator lattice, part of the C ABI of liblt_lattice.so.
 * include/lt_lattice.h includes this header (and this one includes it, for
 * lt_graph / lt_table_problem and the conventions: device pointers, stream
 * ordering, LT_E* return codes), so either include gives the whole ABI.
 */
#ifndef LT_BEAM_H_
#define LT_BEAM_H_

#include "lt_lattice.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Frame-synchronous beam search over label prefixes: hypotheses that share a
 * label sequence are one hypothesis, whose score (+)-sums its alignments. Any
 * next-state table (FullNGram through its next_state_table()) x
 * FrameDependent. expansions >= 1 (FrameLabelDependent) returns
 * LT_EUNSUPPORTED and launches nothing. (+) is logaddexp (LT_SEMIRING_LOG) or
 * max (LT_SEMIRING_MAX: a >= b ? a : b with a the blank candidate). The
 * search is fully specified, so every implementation and every launch
 * geometry gives the same beams (bit for bit in LT_SEMIRING_MAX; in
 * LT_SEMIRING_LOG up to the fp32 accuracy of logaddexp, 1e-6 or so).
 *
 * Hypothesis. A label prefix with a score s (fp32), a context state c, a
 * length n, a 64-bit hash h of the prefix, its parent's hash ph (the prefix
 * without its last label) and its last label y. The empty prefix has h = 0,
 * n = 0, c = 0 (the start state, where lt_table_forward starts), s = 0. The
 * hash of prefix + y is mix(h, y), on unsigned 64-bit values with wrap-around:
 *     z = h ^ (y * 0x9E3779B97F4A7C15)
 *     z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *     z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *     z = z ^ (z >> 31)
 * Two prefixes are the same hypothesis iff their (h, n) agree: a hash
 * collision between prefixes of one length is treated as identity (two such
 * prefixes in one beam, 2^-64 a pair, would be merged wrongly).
 *
 * The beam has K = beam_size slots. Before frame 0 slot 0 holds the empty
 * prefix and slots 1..K-1 are dead. The live slots are always slots 0..m-1.
 * Each live frame t < num_frames[b], with R = V + 1:
 *   Candidates. For each live slot i, cand(i, y) = s_i + W[b,t,c_i,y] for
 *     y = 0 (blank: the prefix stays) and y = 1..V (the prefix grows by y):
 *     one fp32 add each, bf16 weights widened exactly. A sum that is NaN
 *     counts as -inf from here on.
 *   Merge. For each live slot i with n_i >= 1, look for the live slot j with
 *     (h_j, n_j) = (ph_i, n_i - 1): slot i's parent, whose extension by y_i
 *     is slot i's own prefix. If there is one (the lowest j if a collision
 *     gives several), cand(i, 0) <- cand(i, 0) (+) cand(j, y_i), and
 *     cand(j, y_i) is removed.
 *   Select. Among the candidates with score > -inf keep the K best: larger
 *     score first, equal scores to the smaller k = i*R + y. A NaN never
 *     wins. The candidate of rank r becomes slot r: a blank candidate keeps
 *     slot i's (h, ph, n, c, y); an extension gets h = mix(h_i, y), ph = h_i,
 *     n = n_i + 1, c = next_state[c_i, y-1], last label y. The score is the
 *     candidate's. Slots past the number of such candidates are dead.
 *   Trace. trace[b,t,r] = (i << 16) | y, -1 for a dead slot;
 *     step_score[b,t,r] = the slot's score, -inf for a dead slot.
 * Frames t >= num_frames[b] leave the beam alone; their trace / step_score
 * rows are -1 / -inf.
 *
 * Outputs, from the slots after the last live frame, in slot order (so best
 * first):
 *   labels [B,K,T] int64: the prefix's labels at the front, 0 after them;
 *   num_labels [B,K] int32: n; scores [B,K] fp32: s.
 *   A dead slot gives all 0 / 0 / -inf. num_frames = 0 gives the empty
 *   hypothesis with score 0 in slot 0; an utterance whose arcs are all -inf
 *   gives an all-dead beam.
 * The score. LT_SEMIRING_LOG: the log of the summed weight of those
 * alignments of the label sequence that the beam kept; never above the
 * sequence's string forward (lt_table_num_forward, Log) and equal to it when
 * nothing was pruned. LT_SEMIRING_MAX: the weight of the best kept alignment.
 * Neither is normalised: subtract lt_table_forward's log_z for a
 * log-probability.
 *
 *   W [B,T,C,V+1] fp32 / bf16, 16-byte aligned, the 16-byte granule that
 *          holds its last byte readable.
 *   trace [B,T,K] int32, step_score [B,T,K] fp32: optional (NULL). Without
 *          `trace` the backpointers are kept in `workspace`.
 *   workspace: lt_table_beam_search_workspace_bytes() bytes (4*B*T*K, what a
 *          NULL `trace` needs), 4-byte aligned; may be NULL when `trace` is
 *          given.
 * One kernel on `stream` (capturable; no allocation, synchronisation or stream
 * of its own), one wave per utterance with lane r as slot r; the label
 * sequences are read back from the trace in the same launch. While a frame of
 * W is at most 32 KiB whole frames are staged into LDS ahead of the search;
 * larger frames are gathered from memory. Every output element, and every
 * workspace byte the kernel reads, is written by the call; reruns are
 * bit-equal.
 * LT_EINVAL: beam_size < 1, a NULL labels / num_labels / scores, a workspace
 * too small for a NULL trace, a semiring other than LOG / MAX.
 * LT_EUNSUPPORTED: expansions >= 1, beam_size > 64 (one wave), V > 1023, or
 * 2^31 or more elements in a frame of W or in the trace. */
int lt_table_beam_search_workspace_bytes(const lt_graph* g, const lt_table_problem* pb,
                                         int32_t beam_size, size_t* bytes);
int lt_table_beam_search(const lt_graph* g, const lt_table_problem* pb, const void* W,
                         const int32_t* num_frames, int32_t beam_size, int32_t semiring,
                         int64_t* labels /* [B,K,T] */, int32_t* num_labels /* [B,K] */,
                         float* scores /* [B,K] */, int32_t* trace /* [B,T,K], may be NULL */,
                         float* step_score /* [B,T,K], may be NULL */, void* workspace,
                         size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LT_BEAM_H_ */
