// lt_align_post_fld.hip -- lt_align_post.hip's emission posteriors on the
// FrameLabelDependent(K) string lattice: up to K labels a frame, then the
// mandatory blank (include/lt_posterior_fld.h has the definition). Within
// frame t, from alpha_t and from beta_{t+1}:
//   x_0 = alpha_t        x_i[u] = x_{i-1}[u-1] + lex_t[u-1]       (i = 1..K)
//   alpha_{t+1}[u] = blank_t[u] + logsumexp_{i<=K} x_i[u]
//   y_0 = blank_t + beta_{t+1}   y_j[u] = lex_t[u] + y_{j-1}[u+1] (j = 1..K)
//   beta_t[u] = logsumexp_{j<=K} y_j[u]
//   emission[t, u] = sum_{i+j+1<=K} exp(x_i[u] + lex_t[u] + y_j[u+1] - log_prob)
//
// The work split, the prologue, the history, the register rings and the one
// meeting at m = nf/2 are lt_align_post.hip's (string_prologue and
// string_midpoint of lt_string_common.h): alpha_m and beta_m are
// frame-boundary vectors, so log_prob = logsumexp_u(alpha_m[u] + beta_m[u])
// holds unchanged and one value normalises both halves. A history row is
// still ONE vector a frame; both waves read it at their own positions.
//
// The frame step is new. A chain of K shifts (wave_prev of the lane's top
// position per component upward, wave_next of its bottom one downward, plus P
// renormalising adds: split_plus) carries x_i / y_j. Every chain value is an
// exact integer part plus a fraction in [0, 1), like the vectors themselves.
// A sum over chain values is kept as a RUNNING pair (M, S): M the largest
// integer part so far (exact), S = sum exp(value - M) in the linear domain,
// 1 <= S < (K+1) e. Two v_exp_f32 a term and no logarithm; the one logarithm
// of a frame turns the last (M, S) into the next vector (run_split).
//   wave F  runs (M, S) over x_0..x_K: its prefixes ARE the cumulative family
//           Xc_i[u] = logsumexp_{i'<=i} x_i'[u]
//   wave R  runs (M, S) over the shifted-in z_j[u] = y_j[u+1], j < K: its
//           prefixes are Yc_j[u+1], and
//           beta_t[u] = y_0[u] (+) lex_t[u] (x) Yc_{K-1}[u+1]
// Phase 2 holds that family of K (M, S) pairs a position in REGISTERS (every
// loop over the slots is unrolled, so the family is indexed statically: no
// scratch) and recomputes the other direction's chain from the other wave's
// row and the frame's weights, meeting slot ii of the family with chain value
// K-1-ii: K terms a cell, each exp(integer parts cancelling exactly +
// fractions) * S with the exponent <= 0, so nothing overflows and a row may
// sum to K.
//   F:  emission[t, u] = sum_j exp(Xc_{K-1-j}[u] + lex_t[u] + y_j[u+1] - lp)
//   R:  emission[t, u] = sum_i exp(x_i[u] + lex_t[u] + Yc_{K-1-i}[u+1] - lp)
// K = 1, 2, 4 are compiled in (KC = K: no branch in the frame); every other K
// up to 15 runs the KC = 0 kernel, unrolled to 15 slots behind wave-uniform
// `slot < K` branches, with a shorter ring (its frame is long). No atomics: a
// call is deterministic.
#include "lt_string_common.h"

namespace {

constexpr int kFldMaxK = 15;

struct FlArgs {
  const unsigned char* W;
  const int* nfr;
  const int* table;    // [C, V] next state of (p, y)
  const int* labels;   // [B, U]
  const int* nlab;     // [B]
  float* em;           // [B, T, U]
  float* lp;           // [B]
  float2* ws;          // history [B, T, 64P] (integer part, fraction) when not in LDS
  int B, T, U, C, V, R, K;
  int stage_tab;       // the next-state table is staged in LDS for the walk
};

// (o, f) + w with the fraction back in [0, 1); w = -inf: the zero (-inf, 0)
LT_DEVINL void split_plus(float o, float f, float w, float& no, float& nf) {
  const float s = f + w;
  const float fl = floorf(s);
  const bool fin = __builtin_isfinite(s);
  no = fin ? o + fl : s;
  nf = fin ? s - fl : 0.f;
}
// the running sum (M, S) of exp(o + f) terms: M the largest integer part so
// far, S the terms' sum relative to it; the zero is (-inf, 0)
LT_DEVINL void run_first(float o, float f, float& M, float& S) {
  M = o;
  S = o == -kInf ? 0.f : lt_exp(f);
}
LT_DEVINL void run_plus(float o, float f, float& M, float& S) {
  const float Mn = fmaxf(M, o);
  S = Mn == -kInf ? 0.f : S * lt_exp(M - Mn) + lt_exp((o - Mn) + f);
  M = Mn;
}
// (o, f) of w + M + log S
LT_DEVINL void run_split(float M, float S, float w, float& no, float& nf) {
  const float r = w + lt_log_acc(S);
  const float fl = floorf(r);
  const bool zero = M == -kInf, fin = __builtin_isfinite(r);
  no = zero ? M : (fin ? M + fl : r);
  nf = (zero || !fin) ? 0.f : r - fl;
}

// frames of weights / history in flight
template <int P, int KC>
constexpr int fld_depth() {
  return KC == 0 ? 4 : (KC == 4 ? (P == 1 ? 8 : 4) : (P == 1 ? 16 : 8));
}

// Steps i0..i1-1 of one wave; step i is frame t = i (F) or nf-1-i (R). Phase
// 1 (!PH2) stores the wave's vector before each frame into the history,
// phase 2 reads the other wave's row of the frame and stores emission[t, :].
template <bool BF16, int P, int KC, bool REV, bool PH2>
LT_DEVINL void fld_phase(const unsigned char* wbase, long long frame_bytes, const int (&ob)[P],
                         const int (&ol)[P], float (&o)[P], float (&v)[P], float2* hist, float* em,
                         int U, int Krt, int lane, int i0, int i1, int nf, float lpi, float lpf) {
  constexpr int SP = 64 * P;
  constexpr int D = fld_depth<P, KC>();
  constexpr int KM = KC ? KC : kFldMaxK;  // slots the loops are unrolled to
  const int K = KC ? KC : Krt;
  if (i0 >= i1) return;
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
      if constexpr (PH2) ph[d][j] = hist[(long long)t * SP + lane * P + j];
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
          if constexpr (PH2) ph[d][j] = hist[(long long)tn * SP + lane * P + j];
        }
      }
      if constexpr (!PH2) {
        float2* hr = hist + (long long)t * SP + lane * P;
#pragma unroll
        for (int j = 0; j < P; ++j) hr[j] = make_float2(o[j], v[j]);
      }
      float* er = em + (long long)t * U;
      // the family phase 2 holds across the frame: slot s is Xc_s[u] (F) or
      // Yc_s[u+1] (R) as a running pair
      float fM[PH2 ? KM : 1][P], fS[PH2 ? KM : 1][P];
      float M[P], S[P], acc[P];
      (void)fM, (void)fS, (void)acc;
      if constexpr (!REV) {
        // ---- x_0..x_K upward; (M, S) runs over them
        float xo[P], xf[P];
#pragma unroll
        for (int j = 0; j < P; ++j) {
          xo[j] = o[j];
          xf[j] = v[j];
          run_first(xo[j], xf[j], M[j], S[j]);
        }
#pragma unroll
        for (int s = 0; s < KM; ++s) {
          if (s >= K) continue;
          float so[P], sf[P];
#pragma unroll
          for (int j = 0; j < P; ++j) {
            if constexpr (PH2) {
              fM[s][j] = M[j];
              fS[s][j] = S[j];
            }
            split_plus(xo[j], xf[j], wl[j], so[j], sf[j]);  // the arc leaving u
          }
          const float po = wave_prev(so[P - 1], -kInf), pf = wave_prev(sf[P - 1], 0.f);
#pragma unroll
          for (int j = 0; j < P; ++j) {
            xo[j] = j ? so[j ? j - 1 : 0] : po;
            xf[j] = j ? sf[j ? j - 1 : 0] : pf;
            run_plus(xo[j], xf[j], M[j], S[j]);
          }
        }
        if constexpr (PH2) {
          // ---- y_0..y_{K-1} downward from the row beta_{t+1}; z = y_j[u+1]
          // meets Xc_{K-1-j}[u]
          float yo[P], yf[P];
#pragma unroll
          for (int j = 0; j < P; ++j) {
            split_plus(hh[j].x, hh[j].y, wb[j], yo[j], yf[j]);
            acc[j] = 0.f;
          }
#pragma unroll
          for (int s = KM - 1; s >= 0; --s) {
            if (s >= K) continue;
            const float nxo = wave_next(yo[0], -kInf), nxf = wave_next(yf[0], 0.f);
#pragma unroll
            for (int j = 0; j < P; ++j) {
              const int u = lane * P + j;
              // none leaves position U
              const float zo = u < U ? (j == P - 1 ? nxo : yo[j == P - 1 ? j : j + 1]) : -kInf;
              const float zf = u < U ? (j == P - 1 ? nxf : yf[j == P - 1 ? j : j + 1]) : 0.f;
              const float arg = (zo + fM[s][j] - lpi) + (zf + wl[j] - lpf);
              acc[j] += lt_exp(arg) * fS[s][j];
              if (s > 0) split_plus(zo, zf, wl[j], yo[j], yf[j]);
            }
          }
        }
#pragma unroll
        for (int j = 0; j < P; ++j) run_split(M[j], S[j], wb[j], o[j], v[j]);
      } else {
        // ---- y_0..y_K downward; (M, S) runs over z_j[u] = y_j[u+1], j < K
        float y0o[P], y0f[P], yo[P], yf[P];
#pragma unroll
        for (int j = 0; j < P; ++j) {
          split_plus(o[j], v[j], wb[j], y0o[j], y0f[j]);
          yo[j] = y0o[j];
          yf[j] = y0f[j];
          M[j] = -kInf;
          S[j] = 0.f;
        }
#pragma unroll
        for (int s = 0; s < KM; ++s) {
          if (s >= K) continue;
          const float nxo = wave_next(yo[0], -kInf), nxf = wave_next(yf[0], 0.f);
#pragma unroll
          for (int j = 0; j < P; ++j) {
            const int u = lane * P + j;
            // none leaves position U
            const float zo = u < U ? (j == P - 1 ? nxo : yo[j == P - 1 ? j : j + 1]) : -kInf;
            const float zf = u < U ? (j == P - 1 ? nxf : yf[j == P - 1 ? j : j + 1]) : 0.f;
            if (s == 0) run_first(zo, zf, M[j], S[j]);
            else run_plus(zo, zf, M[j], S[j]);
            if constexpr (PH2) {
              fM[s][j] = M[j];
              fS[s][j] = S[j];
            }
            if (s + 1 < K) split_plus(zo, zf, wl[j], yo[j], yf[j]);
          }
        }
        if constexpr (PH2) {
          // ---- x_0..x_{K-1} upward from the row alpha_t; x_i[u] meets
          // Yc_{K-1-i}[u+1]
          float xo[P], xf[P];
#pragma unroll
          for (int j = 0; j < P; ++j) {
            xo[j] = hh[j].x;
            xf[j] = hh[j].y;
            acc[j] = 0.f;
          }
#pragma unroll
          for (int s = KM - 1; s >= 0; --s) {
            if (s >= K) continue;
#pragma unroll
            for (int j = 0; j < P; ++j) {
              const float arg = (xo[j] + fM[s][j] - lpi) + (xf[j] + wl[j] - lpf);
              acc[j] += lt_exp(arg) * fS[s][j];
            }
            if (s > 0) {
              float so[P], sf[P];
#pragma unroll
              for (int j = 0; j < P; ++j) split_plus(xo[j], xf[j], wl[j], so[j], sf[j]);
              const float po = wave_prev(so[P - 1], -kInf), pf = wave_prev(sf[P - 1], 0.f);
#pragma unroll
              for (int j = 0; j < P; ++j) {
                xo[j] = j ? so[j ? j - 1 : 0] : po;
                xf[j] = j ? sf[j ? j - 1 : 0] : pf;
              }
            }
          }
        }
        // beta_t[u] = y_0[u] (+) lex_t[u] (x) Yc_{K-1}[u+1]
#pragma unroll
        for (int j = 0; j < P; ++j) {
          float lo, lf;
          run_split(M[j], S[j], wl[j], lo, lf);
          lae_split(y0o[j], y0f[j], lo, lf, o[j], v[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < P; ++j) {
        const int u = lane * P + j;
        if constexpr (PH2)
          if (u < U) er[u] = acc[j];
        if (u > U) {
          o[j] = -kInf;
          v[j] = 0.f;
        }
      }
    }
  }
}

template <bool BF16, int P, int KC, bool HL>
__global__ __launch_bounds__(128) void align_post_fld_kernel(const FlArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fl_sm[];
  constexpr int SP = 64 * P;  // string positions a wave holds
  constexpr int ES = BF16 ? 2 : 4;
  const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.x;
  const bool rev = __builtin_amdgcn_readfirstlane(tid) >= 64;  // wave R
  const int U = a.U, T = a.T, K = a.K;
  int nf = a.nfr[b];
  nf = nf < 0 ? 0 : (nf > T ? T : nf);
  float* em = a.em + (long long)b * T * U;

  // ---- rows of padding frames
  for (long long i = (long long)nf * U + tid; i < (long long)T * U; i += 128) em[i] = 0.f;

  // ---- string positions: context state and label class
  int ob[P], ol[P];
  const StringLds sl = string_prologue<P, 128, 16>(a, b, tid, lane, fl_sm, ob, ol);
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
  if (!rev) fld_phase<BF16, P, KC, false, false>(wbase, FRB, ob, ol, o, v, hist, em, U, K, lane, 0, n1, nf, 0.f, 0.f);
  else fld_phase<BF16, P, KC, true, false>(wbase, FRB, ob, ol, o, v, hist, em, U, K, lane, 0, n1, nf, 0.f, 0.f);

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
  if (!rev) fld_phase<BF16, P, KC, false, true>(wbase, FRB, ob, ol, o, v, hist, em, U, K, lane, n1, nf, nf, lpi, lpf);
  else fld_phase<BF16, P, KC, true, true>(wbase, FRB, ob, ol, o, v, hist, em, U, K, lane, n1, nf, nf, lpi, lpf);
}

// Validates the shape and lays out LDS / workspace.
int fld_plan(const lt_graph* g, const lt_table_problem* pb, StringPlan* pl) {
  if (int rc = table_check("lt_table_align_posteriors_fld", g, pb, kChkString, [&] {
        if (g->expansions < 1)
          return fail(LT_EUNSUPPORTED,
                      "lt_table_align_posteriors_fld: FrameDependent (expansions == 0)");
        if (g->expansions > kFldMaxK)
          return fail(LT_EUNSUPPORTED, "lt_table_align_posteriors_fld: expansions > 15");
        if (pb->max_labels > 255)
          return fail(LT_EUNSUPPORTED, "lt_table_align_posteriors_fld: max_labels > 255");
        return LT_OK;
      }))
    return rc;
  pl->P = string_positions(pb->max_labels);
  const long long SP = 64LL * pl->P;
  // ctx, yn, yt; alpha_m, beta_m; a frame of history is (integer part, fraction) a position
  string_layout(g, pb, 3 * 4 * SP + 2 * 8 * SP, 8 * SP, 0, pl);
  return LT_OK;
}

template <int KC>
int fld_launch(const StringPlan& pl, bool bf16, const FlArgs& a, hipStream_t st) {
  return dispatch(bf16, pl.P, [&](auto bf, auto p) {
    constexpr bool BF16 = decltype(bf)::value;
    constexpr int P = decltype(p)::value;
    auto k = pl.hist_lds ? align_post_fld_kernel<BF16, P, KC, true>
                         : align_post_fld_kernel<BF16, P, KC, false>;
    return launch(k, dim3(a.B), dim3(128), pl.lds, st, a, "FrameLabelDependent alignment posteriors");
  });
}

}  // namespace

extern "C" {

int lt_table_align_posteriors_fld_workspace_bytes(const lt_graph* g, const lt_table_problem* pb,
                                                  size_t* bytes) {
  StringPlan pl;
  if (int rc = fld_plan(g, pb, &pl)) return rc;
  if (bytes) *bytes = pl.ws;
  return LT_OK;
}

int lt_table_align_posteriors_fld(const lt_graph* g, const lt_table_problem* pb, const void* W,
                                  const int32_t* num_frames, const int32_t* labels,
                                  const int32_t* num_labels, float* emission, float* log_prob,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  StringPlan pl;
  if (int rc = fld_plan(g, pb, &pl)) return rc;
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
  FlArgs a;
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
  a.K = g->expansions;
  a.stage_tab = pl.stage_tab;
  hipStream_t st = (hipStream_t)stream;
  switch (a.K) {
    case 1: return fld_launch<1>(pl, bf16, a, st);
    case 2: return fld_launch<2>(pl, bf16, a, st);
    case 4: return fld_launch<4>(pl, bf16, a, st);
    default: return fld_launch<0>(pl, bf16, a, st);
  }
}

}  // extern "C"
