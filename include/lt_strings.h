/*
 * lt_strings.h -- the weights of N label strings per utterance on the
 * utterance's one W (N-best rescoring), and the dense arc-weight gradient of
 * any linear combination of them (N-best minimum-risk training). Part of the
 * C ABI of liblt_lattice.so. include/lt_lattice.h includes this header (and
 * this one includes it, for lt_graph / lt_table_problem and the conventions:
 * device pointers, stream ordering, LT_E* return codes), so either include
 * gives the whole ABI.
 */
#ifndef LT_STRINGS_H_
#define LT_STRINGS_H_

#include "lt_lattice.h"

#ifdef __cplusplus
extern "C" {
#endif

/* For utterance b and hypothesis n < num_hyps, with the labels
 * labels[b, n, :U] (U = pb->max_labels), nl = num_labels[b, n] and nf =
 * num_frames[b] (clamped to [0, T]), on the string lattice of lt_posterior.h
 * over utterance b's W (every hypothesis of an utterance reads the same W):
 *   score[b, n] = log_prob of lt_posterior.h = alpha_nf[nl] of the Log string
 *                 recursion (= lt_table_num_forward in LT_SEMIRING_LOG).
 *   - labels outside 1..V are epsilons, as in lt_posterior.h: they read label
 *     1's weight and keep the context state.
 *   - num_labels outside [0, U], or no path of finite weight: -inf, never NaN.
 *   - nf = 0 with nl = 0: 0.
 * Gradient, given grad [B, N] fp32 (d objective / d score):
 *   dW[b, t, ctx_u, 0]       += grad[b,n] * blank_occ_n[t,u]   (u <= nl)
 *   dW[b, t, ctx_u, y_{u+1}] += grad[b,n] * emission_n[t,u]    (u <  nl)
 * with emission and blank_occ of hypothesis n as lt_string_expect.h defines
 * them; every other element of dW [B,T,C,V+1] (fp32) is 0, rows t >= nf are
 * 0, and a hypothesis with score -inf or grad 0 contributes nothing. Every
 * element of dW is written by the kernel (no memset). A non-finite grad[b, n]
 * makes every element of utterance b's live rows NaN.
 *
 * lt_table_strings_forward: ONE kernel on `stream` (capturable; no allocation,
 * synchronisation or stream of its own). Grid (utterance, group of 8
 * hypotheses, direction); one wave is one hypothesis, and the 8 waves of a
 * workgroup share the frames of W, which the workgroup stages a slice ahead
 * into a two-slice LDS ring (a slice: the most whole frames that fit 32 KiB,
 * at most 64; a frame larger than that is read from memory by each wave).
 * Direction 0 is alpha and writes score. With want_history != 0 direction 1
 * (beta) runs too, and both write to `workspace` what the backward reads: per
 * frame and hypothesis the row of SP = 64 * ceil((U+1)/64) (rounded up to 64,
 * 128 or 256) fp32 values relative to the row's integer offset and that
 * offset, per hypothesis the cell indices of its positions and its score as
 * (offset, fraction). Without want_history nothing but score is written and
 * the workspace may be NULL.
 *
 * lt_table_strings_backward: ONE kernel, frame-parallel, no recursion: a
 * workgroup owns a block of frames of one utterance and, per frame, zeroes a
 * 64-bit integer image of the frame in LDS, adds every term
 *   grad_n * exp((offsets) + (fractions))   converted to fixed point
 * into its cell with an LDS 64-bit integer add, and behind a barrier converts
 * the image to fp32 and stores the frame, zeros included. The fixed-point
 * scale is a power of two per utterance: with m = max_n |grad[b,n]| < 2^e and
 * c = ceil(log2(2 N (U+1))) it is 2^(62 - c - e), so the 2 N (U+1) terms of
 * a frame cannot overflow 63 bits and the quantum is at most 2^-46 m. Integer
 * addition is associative: dW does not depend on the order in which waves
 * arrive, two calls give bit-equal outputs, and dW is the exact sum of its
 * fp32 terms rounded once. No float atomics. `score` must be the forward's
 * output and `workspace` the one a forward with want_history filled for the
 * same arguments.
 *
 * Range: FrameDependent (expansions == 0), any next-state table, fp32 or bf16
 * W (16-byte aligned), 1 <= num_hyps <= 64, max_labels <= 255, fewer than
 * 2^31 weights per frame; the backward also needs its LDS image:
 *   8 * C * (V+1) + 1280 <= 160 KiB   (C * (V+1) <= 20320 cells).
 * Outside it LT_EUNSUPPORTED -- from lt_table_strings_workspace_bytes for the
 * forward's range, from lt_table_strings_backward (also on an empty batch,
 * before any pointer is looked at) for its LDS rule -- and nothing is launched.
 * Workspace: lt_table_strings_workspace_bytes() bytes, 16-byte aligned:
 *   2 * 4 * B N T SP (the two histories) + 2 * 4 * B N T (row offsets)
 *   + 8 * B N SP (cell indices) + 8 * B N (scores), each part rounded up to
 *   256 bytes. in_offsets / in_arcs of *g are not read. */
int lt_table_strings_workspace_bytes(const lt_graph* g, const lt_table_problem* pb,
                                     int32_t num_hyps, size_t* bytes);
int lt_table_strings_forward(const lt_graph* g, const lt_table_problem* pb, const void* W,
                             const int32_t* num_frames, int32_t num_hyps,
                             const int32_t* labels /* [B,N,U] */,
                             const int32_t* num_labels /* [B,N] */, float* score /* [B,N] */,
                             void* workspace, size_t workspace_bytes, int32_t want_history,
                             void* stream);
int lt_table_strings_backward(const lt_graph* g, const lt_table_problem* pb, const void* W,
                              const int32_t* num_frames, int32_t num_hyps,
                              const int32_t* labels /* [B,N,U] */,
                              const int32_t* num_labels /* [B,N] */,
                              const float* score /* [B,N] */, const float* grad /* [B,N] */,
                              float* dW /* [B,T,C,V+1] */, void* workspace,
                              size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LT_STRINGS_H_ */
