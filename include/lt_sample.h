/*
 * lt_sample.h -- sampling alignment paths from the lattice posterior, part of
 * the C ABI of liblt_lattice.so. include/lt_lattice.h includes this header
 * (and this one includes it, for lt_graph / lt_table_problem and the
 * conventions: device pointers, stream ordering, LT_E* return codes), so
 * either include gives the whole ABI.
 */
#ifndef LT_SAMPLE_H_
#define LT_SAMPLE_H_

#include "lt_lattice.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Draws num_samples paths per utterance from p(pi) = exp(w(pi)) / Z of the
 * denominator lattice (all label sequences): any next-state table (FullNGram
 * through its next_state_table()) x FrameDependent. expansions >= 1
 * (FrameLabelDependent) returns LT_EUNSUPPORTED and launches nothing.
 *
 * A path takes one arc per live frame t < num_frames[b]: blank (y = 0, the
 * state stays) or label y (state -> next_state[p, y-1]); it starts at state
 * 0, where lt_table_forward starts. The draw is Gumbel-max on a counter-based
 * generator, walked backwards over alpha; it is fully specified, so every
 * device and every launch geometry gives the same paths for the same seed.
 *
 * Noise. For utterance b, sample s, frame t and arc (p, y), let
 * k = p*(V+1) + y.
 *   - Run Philox4x32-10 (Random123's constants and round function) with
 *       key = (seed & 0xffffffff, seed >> 32),
 *       counter = (k >> 2, t, s, b).
 *   - Take output word r = out[k & 3].
 *   - u = ((r >> 8) + 0.5) * 2^-24, strictly inside (0, 1). It is an fp32
 *     number while r >> 8 < 2^23; above that 1 - u is one, and -log u is
 *     taken as -log1p(-(1 - u)), so no u rounds to 1.
 *   - g(b, s, t, p, y) = -log(-log u), computed in fp32 with ordinary logf
 *     accuracy: -2.86 <= g <= 17.33, and an implementation's g is within a
 *     few 1e-6 of the real one (the kernel's v_log_f32 form: 1.8e-6).
 *   - The noise of an arc does not depend on the CSR order, on how many
 *     samples the call draws, or on which wave handles it.
 * Last live frame t = nf-1: take the arc maximising
 *   alpha_t[p] + W[b,t,p,y] + g over all C*(V+1) arcs of the frame; its
 *   source p becomes the current state q.
 * Every earlier frame t, with q the state before frame t+1: among the arcs
 *   into q -- the blank arc (q, 0) and the in-arcs (p, y) with
 *   next_state[p, y-1] = q -- take the one maximising the same score; its
 *   source becomes q.
 * Ties go to the smallest k. Scores are fp32 sums, alpha + W first and then
 * + g; bf16 weights are widened exactly. A score that is NaN never wins.
 * Because every arc into a state of finite alpha has a finite score, a
 * sampled path has finite weight when log Z is finite.
 * Degenerate utterances: num_frames = 0 gives the empty path (labels all 0,
 * weight 0); a log_z that is not finite makes the utterance unsampled
 * (labels all 0, weight -inf).
 *
 *   log_z [B], alpha [B,T,C]: what lt_table_forward or lt_den_forward wrote
 *          in LT_SEMIRING_LOG. Like W, alpha is 16-byte aligned and the
 *          16-byte granule that holds its last byte is readable.
 *   labels [B,S,T] int64: the true label y of the arc taken on frame t
 *          (0 = blank), 0 on padding frames.
 *   path_weight [B,S]: the fp32 sum of the path's arc weights, added from the
 *          last frame to the first.
 * One kernel on `stream` (capturable; no allocation, synchronisation or
 * stream of its own), one wave per (utterance, sample). While a frame of W
 * and alpha fits a staging slice (at most 32 KiB, lt_sample.hip) whole frames
 * are staged into LDS ahead of the walk; larger frames are gathered from
 * memory, one dependent access per step. `workspace` is not used today:
 * lt_table_sample_workspace_bytes() returns 0 and it may be NULL.
 * num_samples < 1 or a NULL output: LT_EINVAL. Fewer than 2^31 weights per
 * frame and num_samples * batch < 2^31, else LT_EUNSUPPORTED. */
int lt_table_sample_workspace_bytes(const lt_graph* g, const lt_table_problem* pb,
                                    int32_t num_samples, size_t* bytes);
int lt_table_sample(const lt_graph* g, const lt_table_problem* pb, const void* W,
                    const int32_t* num_frames, const float* log_z /* [B] */,
                    const float* alpha /* [B,T,C], Log */, int32_t num_samples, uint64_t seed,
                    int64_t* labels /* [B,S,T]: true label y, 0 = blank, 0 on padding frames */,
                    float* path_weight /* [B,S]: fp32 sum of the path's arc weights */,
                    void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LT_SAMPLE_H_ */
