/*
 * lt_paths.h -- scoring given alignment paths, scattering per-path gradients
 * onto their arcs, and the edit distance of hypotheses against references:
 * the three operations behind RecognitionLattice.path_weights and
 * sampled_risk. Part of the C ABI of liblt_lattice.so. include/lt_lattice.h
 * includes this header (and this one includes it, for lt_graph /
 * lt_table_problem and the conventions: device pointers, stream ordering,
 * LT_E* return codes), so either include gives the whole ABI.
 */
#ifndef LT_PATHS_H_
#define LT_PATHS_H_

#include "lt_lattice.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The weight of given paths through the denominator lattice: any next-state
 * table (FullNGram through its next_state_table()) x FrameDependent.
 * expansions >= 1 (FrameLabelDependent) returns LT_EUNSUPPORTED and launches
 * nothing.
 *
 *   labels [B,S,T] int64: lt_table_sample's layout, the true label y of the
 *          arc a path takes on frame t (0 = blank). Labels on padding frames
 *          t >= num_frames[b] are ignored.
 *   path_weight [B,S] fp32, states [B,S,T] int32 (may be NULL).
 *
 * A path starts in state q_0 = 0. On each live frame t < num_frames[b]
 * (clamped to [0, T]) it takes arc (q_t, y_t); q_{t+1} = q_t if y_t = 0, else
 * next_state[q_t, y_t - 1].
 *   - path_weight is the fp32 sum of W[b,t,q_t,y_t] (bf16 widened exactly),
 *     started at 0 and added from the LAST live frame to the FIRST: the order
 *     lt_sample.h fixes, so scoring the labels lt_table_sample returned gives
 *     its path_weight bit for bit.
 *   - states[b,s,t] = q_t on the live frames of a valid path, -1 everywhere
 *     else (padding frames, invalid paths).
 *   - A live label outside [0, V] makes the path invalid: weight -inf (never
 *     NaN), states all -1.
 *   - num_frames = 0: weight 0.
 * Every element of both outputs is written.
 *
 * One kernel on `stream` (capturable; no allocation, no synchronisation, no
 * workspace), one wave per (utterance, path). The state walk is the only
 * serial part: 64 labels are loaded coalesced, the non-blank lanes balloted,
 * and only those stepped over, through the table in LDS while its 4*C*V bytes
 * are at most 64 KiB and through memory past that. Every lane then gathers
 * its own frame's weight into an LDS row of the path, and the ordered sum
 * runs over that row. The rows bound T: 4 * ceil64(T) bytes must fit the
 * 160 KiB of LDS (next to the table while both fit), i.e. T <= 40960;
 * longer problems return LT_EUNSUPPORTED.
 *
 * num_paths < 1 or a NULL required pointer: LT_EINVAL. C*(V+1) >= 2^31 or
 * num_paths * batch >= 2^31: LT_EUNSUPPORTED. All validation precedes the
 * launch. batch = 0 is a successful no-op. */
int lt_table_path_score(const lt_graph* g, const lt_table_problem* pb, const void* W,
                        const int32_t* num_frames, const int64_t* labels /* [B,S,T] */,
                        int32_t num_paths, float* path_weight /* [B,S] */,
                        int32_t* states /* [B,S,T] or NULL */, void* stream);

/* Scatters one scalar per path onto the arcs the path takes:
 *   dW[b,t,q,y] = sum_s grad[b,s] * 1[states[b,s,t] = q and labels[b,s,t] = y]
 * as dense fp32 [B,T,C,V+1] (W's shape; pb->weight_dtype is not used), every
 * other element exactly 0. `states` is what lt_table_path_score wrote for
 * `labels`: a negative state (padding, invalid path) contributes nothing, and
 * neither does a frame t >= num_frames[b], a state >= C or a label outside
 * [0, V]. The sum over s is taken in ascending s, started at 0.
 *
 * One kernel on `stream` (capturable), the zeros included, as in
 * lt_table_string_scatter: a workgroup stores zeros over the 64 frames of dW
 * it owns and, behind a barrier, one thread per (b, t) column loops over s,
 * so paths that share an arc add in a fixed order: no atomics, bit-equal
 * reruns. Same graphs, range and validation as lt_table_path_score (T is not
 * bounded here). */
int lt_table_path_scatter(const lt_graph* g, const lt_table_problem* pb,
                          const int32_t* num_frames, const int64_t* labels /* [B,S,T] */,
                          const int32_t* states /* [B,S,T] */, int32_t num_paths,
                          const float* grad /* [B,S] */, float* dW /* [B,T,C,V+1] */,
                          void* stream);

/* Unit-cost Levenshtein distance of each hypothesis against its utterance's
 * reference.
 *
 *   hyp [B,S,T] int64, num_frames [B] (NULL: every hypothesis has T frames),
 *   ref [B,U] int32, num_labels [B],
 *   distance [B,S] int32, hyp_length [B,S] int32 (may be NULL).
 *
 * Tokens are the values > 0; values <= 0 are skipped in both sequences
 * (blanks in an alignment, zero epsilons in a transcript). hyp positions
 * t >= num_frames[b] (clamped to [0, T]) and ref positions u >= num_labels[b]
 * are ignored. distance is the Levenshtein distance (substitution, insertion
 * and deletion each cost 1) between the two token sequences, an exact
 * integer; hyp_length is the hypothesis's token count. num_labels[b] outside
 * [0, U] gives distance -1 for that utterance (hyp_length is still the count).
 *
 * One kernel on `stream` (capturable; no allocation, synchronisation or
 * workspace), one wave per (utterance, hypothesis). The DP row over the
 * reference positions 0..n lives in registers, P consecutive cells a lane
 * (P = 1, 2, 4, 8 or 16: the smallest with 64 P >= U + 1). Each hypothesis
 * token h is one row update,
 *   tmp[j] = min(D[j] + 1, D[j-1] + [ref_j != h]),
 *   D'[j]  = j + min_{k <= j} (tmp[k] - k)      (the insertion chain),
 * the second line a prefix-min scan over the wave.
 *
 * max_labels + 1 > 1024 cells: LT_EUNSUPPORTED. num_hyps < 1, a negative
 * shape or a NULL required pointer: LT_EINVAL. num_hyps * batch >= 2^31:
 * LT_EUNSUPPORTED. All validation precedes the launch. batch = 0 is a
 * successful no-op. */
int lt_edit_distance(int32_t batch, int32_t num_hyps, int32_t max_frames, int32_t max_labels,
                     const int64_t* hyp /* [B,S,T] */, const int32_t* num_frames /* [B] or NULL */,
                     const int32_t* ref /* [B,U] */, const int32_t* num_labels /* [B] */,
                     int32_t* distance /* [B,S] */, int32_t* hyp_length /* [B,S] or NULL */,
                     void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LT_PATHS_H_ */
