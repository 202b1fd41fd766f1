// lt_align_post.hip -- per-label emission posteriors of a label string: the
// Log-semiring sibling of lt_align.hip. For the string lattice of
// RecognitionLattice._string_forward (FrameDependent, any next-state table)
//   emission[t, u] = exp(alpha_t[u] + lex_t[u] + beta_{t+1}[u+1] - log_prob)
// the posterior probability that the arc leaving string position u is taken
// on frame t (include/lt_posterior.h has the definition), in ONE launch.
//
// One 128-thread workgroup per utterance: wave F runs alpha upward from frame
// 0, wave R runs beta downward from frame nf-1, and they meet once, at the
// midpoint m = nf/2.
//   prologue   string_prologue (lt_string_common.h): labels to LDS, one lane
//              walks the context states (the table staged in LDS while it is
//              small), every lane of both waves keeps the two weight offsets
//              of its P = ceil((U+1)/64) consecutive positions in registers
//   phase 1    F stores alpha_t for t < m, R stores beta_{t+1} for t >= m
//              into the history [T, 64P] (one row per frame, written by
//              exactly one of the two) -- in LDS while T rows fit beside the
//              prologue's arrays, else in the caller's workspace
//   midpoint   string_midpoint (lt_string_common.h): F publishes alpha_m and R
//              beta_m in LDS, ONE workgroup barrier, then both waves compute
//                  log_prob = logsumexp_u(alpha_m[u] + beta_m[u])
//              from the same LDS words by the same instructions: one value,
//              bit-equal in both waves, normalises both halves
//   phase 2    F has alpha_t in registers for t >= m, reads R's beta_{t+1}
//              and emits frames m..nf-1; R has beta_{t+1} in registers for
//              t < m, reads F's alpha_t and emits frames 0..m-1
// A frame's weights and its history row do not depend on the recursion: both
// are loaded kD frames ahead through register rings, so no global load sits
// on the chain. Every position is an exact integer part plus a fraction in
// [0, 1) (lae_split, lt_kernels.h) in registers AND in the history: the
// exponent's three large terms cancel exactly in the integer parts and only
// fractions are rounded. No atomics: a call is deterministic.
#include "lt_string_common.h"

namespace {

struct PoArgs {
  const unsigned char* W;
  const int* nfr;
  const int* table;    // [C, V] next state of (p, y)
  const int* labels;   // [B, U]
  const int* nlab;     // [B]
  float* em;           // [B, T, U]
  float* lp;           // [B]
  float2* ws;          // history [B, T, 64P] (integer part, fraction) when not in LDS
  int B, T, U, C, V, R;
  int stage_tab;       // the next-state table is staged in LDS for the walk
};

// Steps i0..i1-1 of one wave; step i is frame t = i (F) or nf-1-i (R). Phase
// 1 (!PH2) stores the wave's vector before each frame into the history,
// phase 2 reads the other wave's row of the frame and stores emission[t, :].
template <bool BF16, int P, bool REV, bool PH2>
LT_DEVINL void post_phase(const unsigned char* wbase, long long frame_bytes, const int (&ob)[P],
                          const int (&ol)[P], float (&o)[P], float (&v)[P], float2* hist,
                          float* em, int U, int lane, int i0, int i1, int nf, float lpi,
                          float lpf) {
  constexpr int SP = 64 * P;
  constexpr int D = P == 1 ? 16 : 8;  // frames of weights / history in flight
  if (i0 >= i1) return;
  // F reads beta_{t+1}[u+1], R reads alpha_t[u] (column SP-1 is never a live arc)
  int hx[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int u = lane * P + j;
    hx[j] = REV ? u : (u + 1 < SP ? u + 1 : SP - 1);
  }
  float pb[D][P], pl[D][P];
  float2 ph[D][P];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const int i = i0 + d < i1 ? i0 + d : i1 - 1;
    const int t = REV ? nf - 1 - i : i;
    const unsigned char* wf = wbase + (long long)t * frame_bytes;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      pb[d][j] = ldw<BF16>(wf, ob[j]);
      pl[d][j] = ldw<BF16>(wf, ol[j]);
      if constexpr (PH2) ph[d][j] = hist[(long long)t * SP + hx[j]];
    }
  }
  for (int ib = i0; ib < i1; ib += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int i = ib + d;
      if (i >= i1) break;
      const int t = REV ? nf - 1 - i : i;
      float wb[P], wl[P];
      float2 hh[P];
#pragma unroll
      for (int j = 0; j < P; ++j) {
        wb[j] = pb[d][j];
        wl[j] = pl[d][j];
        if constexpr (PH2) hh[j] = ph[d][j];
      }
      {
        const int in = i + D < i1 ? i + D : i1 - 1;
        const int tn = REV ? nf - 1 - in : in;
        const unsigned char* wf = wbase + (long long)tn * frame_bytes;
#pragma unroll
        for (int j = 0; j < P; ++j) {
          pb[d][j] = ldw<BF16>(wf, ob[j]);
          pl[d][j] = ldw<BF16>(wf, ol[j]);
          if constexpr (PH2) ph[d][j] = hist[(long long)tn * SP + hx[j]];
        }
      }
      if constexpr (!PH2) {
        float2* hr = hist + (long long)t * SP + lane * P;
#pragma unroll
        for (int j = 0; j < P; ++j) hr[j] = make_float2(o[j], v[j]);
      }
      float* er = em + (long long)t * U;
      float no[P], nv[P];
      if constexpr (!REV) {
        // the arc leaving u: (o[j], lv[j]) = alpha_t[u] + lex_t[u]
        float lv[P];
#pragma unroll
        for (int j = 0; j < P; ++j) lv[j] = v[j] + wl[j];
        if constexpr (PH2) {
#pragma unroll
          for (int j = 0; j < P; ++j) {
            const int u = lane * P + j;
            const float arg = (o[j] + hh[j].x - lpi) + (lv[j] + hh[j].y - lpf);
            if (u < U) er[u] = lt_exp(arg);
          }
        }
        const float po = wave_prev(o[P - 1], -kInf), pv = wave_prev(lv[P - 1], 0.f);
#pragma unroll
        for (int j = 0; j < P; ++j) {
          const int u = lane * P + j;
          const float lo = j ? o[j ? j - 1 : 0] : po, lf = j ? lv[j ? j - 1 : 0] : pv;
          lae_split(o[j], v[j] + wb[j], lo, lf, no[j], nv[j]);
          if (u > U) {
            no[j] = -kInf;
            nv[j] = 0.f;
          }
        }
      } else {
        const float nxo = wave_next(o[0], -kInf), nxv = wave_next(v[0], 0.f);
#pragma unroll
        for (int j = 0; j < P; ++j) {
          const int u = lane * P + j;
          const float ro = j == P - 1 ? nxo : o[j == P - 1 ? j : j + 1];
          const float rv = j == P - 1 ? nxv : v[j == P - 1 ? j : j + 1];
          // the arc leaving u into beta_{t+1}[u+1]; none leaves position U
          const float to = u < U ? ro : -kInf, tv = wl[j] + rv;
          if constexpr (PH2) {
            const float arg = (hh[j].x + to - lpi) + (hh[j].y + tv - lpf);
            if (u < U) er[u] = lt_exp(arg);
          }
          lae_split(o[j], wb[j] + v[j], to, tv, no[j], nv[j]);
          if (u > U) {
            no[j] = -kInf;
            nv[j] = 0.f;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < P; ++j) {
        o[j] = no[j];
        v[j] = nv[j];
      }
    }
  }
}

template <bool BF16, int P, bool HL>
__global__ __launch_bounds__(128) void align_post_kernel(const PoArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char po_sm[];
  constexpr int SP = 64 * P;  // string positions a wave holds
  constexpr int ES = BF16 ? 2 : 4;
  const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.x;
  const bool rev = __builtin_amdgcn_readfirstlane(tid) >= 64;  // wave R
  const int U = a.U, T = a.T;
  int nf = a.nfr[b];
  nf = nf < 0 ? 0 : (nf > T ? T : nf);
  float* em = a.em + (long long)b * T * U;

  // ---- rows of padding frames
  for (long long i = (long long)nf * U + tid; i < (long long)T * U; i += 128) em[i] = 0.f;

  // ---- string positions: context state and label class
  int ob[P], ol[P];
  const StringLds sl = string_prologue<P, 128, 16>(a, b, tid, lane, po_sm, ob, ol);
  float2* mid = (float2*)sl.mid;  // [2, SP] alpha_m, beta_m; behind them the history

  const long long FRB = (long long)a.C * a.R * ES;
  const unsigned char* wbase = a.W + (long long)b * T * FRB;
  float2* hist;
  if constexpr (HL) hist = (float2*)sl.region;
  else hist = a.ws + (long long)b * T * SP;
  const int nlb = a.nlab[b];
  const int fin = (nlb >= 0 && nlb <= U) ? nlb : -1;
  float o[P], v[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int u = lane * P + j;
    o[j] = (rev ? u == fin : u == 0) ? 0.f : -kInf;
    v[j] = 0.f;
  }
  const int m = nf / 2;
  const int n1 = rev ? nf - m : m;  // steps before the midpoint

  // ---- phase 1
  if (!rev) post_phase<BF16, P, false, false>(wbase, FRB, ob, ol, o, v, hist, em, U, lane, 0, n1, nf, 0.f, 0.f);
  else post_phase<BF16, P, true, false>(wbase, FRB, ob, ol, o, v, hist, em, U, lane, 0, n1, nf, 0.f, 0.f);

  // ---- the one meeting of the two waves: log_prob, the same in both
  float lpi, lpf, unused;
  const bool ok =
      string_midpoint<P, false>(mid, nullptr, rev, lane, o, v, nullptr, lpi, lpf, unused);
  if (tid == 0) a.lp[b] = ok ? lpi + lpf : -kInf;
  if (!ok) {  // unaligned: no path carries weight
    for (long long i = tid; i < (long long)nf * U; i += 128) em[i] = 0.f;
    return;
  }

  // ---- phase 2
  if (!rev) post_phase<BF16, P, false, true>(wbase, FRB, ob, ol, o, v, hist, em, U, lane, n1, nf, nf, lpi, lpf);
  else post_phase<BF16, P, true, true>(wbase, FRB, ob, ol, o, v, hist, em, U, lane, n1, nf, nf, lpi, lpf);
}

// Validates the shape and lays out LDS / workspace.
int post_plan(const lt_graph* g, const lt_table_problem* pb, StringPlan* pl) {
  if (int rc = table_check("lt_table_align_posteriors", g, pb, kChkString, [&] {
        if (g->expansions > 0)
          return fail(LT_EUNSUPPORTED,
                      "lt_table_align_posteriors: FrameLabelDependent (expansions >= 1)");
        if (pb->max_labels > 255)
          return fail(LT_EUNSUPPORTED, "lt_table_align_posteriors: max_labels > 255");
        return LT_OK;
      }))
    return rc;
  pl->P = string_positions(pb->max_labels);
  const long long SP = 64LL * pl->P;
  // ctx, yn, yt; alpha_m, beta_m; a frame of history is (integer part, fraction) a position
  string_layout(g, pb, 3 * 4 * SP + 2 * 8 * SP, 8 * SP, 0, pl);
  return LT_OK;
}

}  // namespace

extern "C" {

int lt_table_align_posteriors_workspace_bytes(const lt_graph* g, const lt_table_problem* pb,
                                              size_t* bytes) {
  StringPlan pl;
  if (int rc = post_plan(g, pb, &pl)) return rc;
  if (bytes) *bytes = pl.ws;
  return LT_OK;
}

int lt_table_align_posteriors(const lt_graph* g, const lt_table_problem* pb, const void* W,
                              const int32_t* num_frames, const int32_t* labels,
                              const int32_t* num_labels, float* emission, float* log_prob,
                              void* workspace, size_t workspace_bytes, void* stream) {
  StringPlan pl;
  if (int rc = post_plan(g, pb, &pl)) return rc;
  if (pb->batch == 0) return LT_OK;
  const bool any_em = pb->max_frames > 0 && pb->max_labels > 0;
  if ((!W && pb->max_frames > 0) || !num_frames || !num_labels || !log_prob ||
      (!emission && any_em) || (pb->max_labels > 0 && !labels))
    return fail(LT_EINVAL, "null pointer");
  const bool bf16 = pb->weight_dtype == LT_DTYPE_BF16;
  if (((uintptr_t)W & (bf16 ? 1 : 3)) || ((uintptr_t)num_frames & 3) || ((uintptr_t)labels & 3) ||
      ((uintptr_t)num_labels & 3) || ((uintptr_t)emission & 3) || ((uintptr_t)log_prob & 3) ||
      ((uintptr_t)workspace & 7))
    return fail(LT_EINVAL, "misaligned pointer");
  if (pl.ws && (!workspace || workspace_bytes < pl.ws))
    return fail(LT_EINVAL, "workspace too small");
  PoArgs a;
  memset(&a, 0, sizeof(a));
  a.W = (const unsigned char*)W;
  a.nfr = num_frames;
  a.table = g->next_state;
  a.labels = labels;
  a.nlab = num_labels;
  a.em = emission;
  a.lp = log_prob;
  a.ws = (float2*)workspace;
  a.B = pb->batch;
  a.T = pb->max_frames;
  a.U = pb->max_labels;
  a.C = g->num_states;
  a.V = g->vocab_size;
  a.R = g->vocab_size + 1;
  a.stage_tab = pl.stage_tab;
  hipStream_t st = (hipStream_t)stream;
  return dispatch(bf16, pl.P, [&](auto bf, auto p) {
    constexpr bool BF16 = decltype(bf)::value;
    constexpr int P = decltype(p)::value;
    auto k = pl.hist_lds ? align_post_kernel<BF16, P, true> : align_post_kernel<BF16, P, false>;
    return launch(k, dim3(a.B), dim3(128), pl.lds, st, a, "alignment posteriors");
  });
}

}  // extern "C"
