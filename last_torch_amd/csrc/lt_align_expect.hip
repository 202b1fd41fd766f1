// lt_align_expect.hip -- expected values over the alignments of a label
// string, with their gradients: lt_align_post.hip's two-wave recursion with
// lt_expect.hip's conditional means carried beside alpha and beta, and the
// deterministic scatter from string coordinates to the dense arc-weight
// gradient. include/lt_string_expect.h has the definition.
//
// lt_table_align_expectation: ONE launch, one 128-thread workgroup per
// utterance. Wave F runs (alpha, abar) upward from frame 0, wave R runs (beta,
// bbar) downward from frame nf-1, and they meet once, at m = nf/2.
//   prologue   string_prologue's (lt_string_common.h), kept as this kernel's
//              own code: labels to LDS, one lane walks the context states,
//              every lane of both waves keeps the two weight offsets of its
//              P = ceil((U+1)/64) positions in registers
//   phase 1    F stores (alpha_t, abar_t) for t < m, R stores (beta_{t+1},
//              bbar_{t+1}) for t >= m into the history [T, 3, 64P]: per
//              position (integer part, fraction) and the mean. A value-only
//              call keeps no history.
//   midpoint   string_midpoint (lt_string_common.h) with the means: both waves
//              publish their vectors in LDS, ONE workgroup barrier,
//              then both compute log_prob = logsumexp_u(alpha_m[u] + beta_m[u])
//              and expected = sum_u p_m[u] (abar_m[u] + bbar_m[u]) from the
//              same LDS words by the same instructions: bit-equal in both
//              waves, so `expected` is known before phase 2 and the
//              covariances come out of the same launch
//   phase 2    F emits frames m..nf-1 from its registers and R's rows, R frames
//              0..m-1 from its registers and F's rows: emission, blank_occ,
//              cov_lex, cov_blank. Both waves read row t at column u; F takes
//              beta_{t+1}[u+1] from the lane above (one DPP shift per
//              component), so the blank arc costs no second history load.
// A frame's weights, its two value rows and its history row do not depend on
// the recursion: all are loaded D frames ahead through register rings. The
// means are conditional means in fp32, combined by the softmax weights the
// log-add already computes (lae_mean); a term of weight -inf is selected out,
// never multiplied, so a NaN value there is harmless. No atomics.
//
// lt_table_string_scatter: one kernel. A workgroup owns kScatFrames rows of
// one utterance's dW: it zeroes them, and behind a workgroup barrier writes
// one sum per chain-head cell (the rule of tab_bwd_num_k0_body, lt_table.hip).
#include "lt_string_common.h"

namespace {

struct XArgs {
  const unsigned char* W;
  const float* lval;   // [B, T, U] lexical values
  const float* bval;   // [B, T, U+1] blank values
  const int* nfr;
  const int* table;    // [C, V] next state of (p, y)
  const int* labels;   // [B, U]
  const int* nlab;     // [B]
  float* expected;     // [B]
  float* lp;           // [B]
  float* em;           // [B, T, U], nullable
  float* bo;           // [B, T, U+1], nullable
  float* cl;           // [B, T, U], nullable
  float* cb;           // [B, T, U+1], nullable
  float* ws;           // history [B, T, 3, 64P] when not in LDS
  int B, T, U, C, V, R;
  int stage_tab;       // the next-state table is staged in LDS for the walk
};

// lae_split (lt_kernels.h) with the conditional means of its two terms: the
// result's mean is the softmax-weighted mean of ma and mb, the weights 1 /
// (1 + e) and e / (1 + e) with e = exp(smaller - larger) the log-add's own.
// A zero term (-inf, or underflowed) is selected out: its mean is not read
// into the arithmetic. Both zero, or a result that is not finite: mean 0.
LT_DEVINL void lae_mean(float ia, float fa, float ma, float ib, float fb, float mb, float& io,
                        float& fo, float& mo) {
  constexpr float ninf = -__builtin_inff();
  ia = fa == ninf ? ninf : ia;  // a masked arc (w = -inf) is the zero term
  ib = fb == ninf ? ninf : ib;
  const bool ab = (ia - ib) + (fa - fb) >= 0.f;
  const float i1 = ab ? ia : ib, f1 = ab ? fa : fb, m1 = ab ? ma : mb;
  const float i2 = ab ? ib : ia, f2 = ab ? fb : fa, m2 = ab ? mb : ma;
  const float d = (i2 - i1) + (f2 - f1);
  const float e = __builtin_amdgcn_exp2f(d * kLog2e);
  const float s = 1.f + e;
  const float r = f1 + lt_log_acc(s);
  const float fl = floorf(r);
  const bool zero = i1 == ninf;
  const bool fin = __builtin_isfinite(r);
  io = zero ? i1 : (fin ? i1 + fl : r);
  fo = (zero || !fin) ? 0.f : r - fl;
  // m1 + (m2 - m1) e / (1 + e): the larger term's mean plus a correction, so
  // the quotient's rounding scales with the difference of the two means, not
  // with their size
  const float mix = e > 0.f ? __builtin_fmaf(m2 - m1, e * __builtin_amdgcn_rcpf(s), m1) : m1;
  mo = (zero || !fin) ? 0.f : mix;
}

// Steps i0..i1-1 of one wave; step i is frame t = i (F) or nf-1-i (R). Phase
// 1 (!PH2) stores the wave's vectors before each frame into the history (when
// `keep`), phase 2 reads the other wave's row of the frame and stores the
// frame's rows of the four outputs.
template <bool BF16, int P, bool REV, bool PH2>
LT_DEVINL void exp_phase(const XArgs& a, const unsigned char* wbase, long long frame_bytes,
                         const float* lvb, const float* bvb, const int (&ob)[P],
                         const int (&ol)[P], float (&o)[P], float (&v)[P], float (&mn)[P],
                         float* hist, long long obl, long long obb, bool keep, int U, int nlc,
                         int lane, int i0, int i1, int nf, float lpi, float lpf, float E) {
  constexpr int SP = 64 * P;
  constexpr int D = P == 1 ? 16 : 8;  // frames of weights / values / history in flight
  if (i0 >= i1) return;
  // value columns this lane reads: lexical u < nl, blank u <= nl (others: 0, not read)
  bool hl[P], hb[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int u = lane * P + j;
    hl[j] = u < nlc;
    hb[j] = u <= nlc;
  }
  float pb[D][P], pl[D][P], qb[D][P], ql[D][P], pm[D][P];
  float2 ph[D][P];
  auto fetch = [&](int d, int t) {
    const unsigned char* wf = wbase + (long long)t * frame_bytes;
    const float* lf = lvb + (long long)t * U;
    const float* bf = bvb + (long long)t * (U + 1);
    const float* hr = hist + (long long)t * 3 * SP;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const int u = lane * P + j;
      pb[d][j] = ldw<BF16>(wf, ob[j]);
      pl[d][j] = ldw<BF16>(wf, ol[j]);
      qb[d][j] = hb[j] ? bf[u] : 0.f;
      ql[d][j] = hl[j] ? lf[u] : 0.f;
      if constexpr (PH2) {
        ph[d][j] = ((const float2*)hr)[u];
        pm[d][j] = hr[2 * SP + u];
      }
    }
  };
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const int i = i0 + d < i1 ? i0 + d : i1 - 1;
    fetch(d, REV ? nf - 1 - i : i);
  }
  for (int ib = i0; ib < i1; ib += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int i = ib + d;
      if (i >= i1) break;
      const int t = REV ? nf - 1 - i : i;
      float wb[P], wl[P], vb[P], vl[P], hm[P];
      float2 hh[P];
#pragma unroll
      for (int j = 0; j < P; ++j) {
        wb[j] = pb[d][j];
        wl[j] = pl[d][j];
        vb[j] = qb[d][j];
        vl[j] = ql[d][j];
        if constexpr (PH2) {
          hh[j] = ph[d][j];
          hm[j] = pm[d][j];
        }
      }
      {
        const int in = i + D < i1 ? i + D : i1 - 1;
        fetch(d, REV ? nf - 1 - in : in);
      }
      if constexpr (!PH2) {
        if (keep) {
          float* hr = hist + (long long)t * 3 * SP;
#pragma unroll
          for (int j = 0; j < P; ++j) {
            ((float2*)hr)[lane * P + j] = make_float2(o[j], v[j]);
            hr[2 * SP + lane * P + j] = mn[j];
          }
        }
      }
      // the frame's rows of the outputs (phase 2)
      float el[P], eb[P], kl[P], kb[P];
      float no[P], nv[P], nm[P];
      if constexpr (!REV) {
        // the arcs leaving u: (o[j], xf) = alpha_t[u] + weight, xm = abar_t[u] + value
        float lf[P], lm[P], bf[P], bm[P];
#pragma unroll
        for (int j = 0; j < P; ++j) {
          lf[j] = v[j] + wl[j];
          lm[j] = mn[j] + vl[j];
          bf[j] = v[j] + wb[j];
          bm[j] = mn[j] + vb[j];
        }
        if constexpr (PH2) {
          // beta_{t+1}[u+1]: the row's next column (column 64P is never a live arc)
          const float nxo = wave_next(hh[0].x, -kInf), nxf = wave_next(hh[0].y, 0.f);
          const float nxm = wave_next(hm[0], 0.f);
#pragma unroll
          for (int j = 0; j < P; ++j) {
            const float ro = j == P - 1 ? nxo : hh[j == P - 1 ? j : j + 1].x;
            const float rf = j == P - 1 ? nxf : hh[j == P - 1 ? j : j + 1].y;
            const float rm = j == P - 1 ? nxm : hm[j == P - 1 ? j : j + 1];
            el[j] = lt_exp((o[j] + ro - lpi) + (lf[j] + rf - lpf));
            kl[j] = el[j] > 0.f ? el[j] * ((lm[j] + rm) - E) : 0.f;
            eb[j] = lt_exp((o[j] + hh[j].x - lpi) + (bf[j] + hh[j].y - lpf));
            kb[j] = eb[j] > 0.f ? eb[j] * ((bm[j] + hm[j]) - E) : 0.f;
          }
        }
        const float po = wave_prev(o[P - 1], -kInf), pf = wave_prev(lf[P - 1], 0.f);
        const float pq = wave_prev(lm[P - 1], 0.f);
#pragma unroll
        for (int j = 0; j < P; ++j) {
          const int u = lane * P + j;
          const float lo = j ? o[j ? j - 1 : 0] : po, lff = j ? lf[j ? j - 1 : 0] : pf;
          const float lmm = j ? lm[j ? j - 1 : 0] : pq;
          lae_mean(o[j], bf[j], bm[j], lo, lff, lmm, no[j], nv[j], nm[j]);
          if (u > U) {
            no[j] = -kInf;
            nv[j] = 0.f;
            nm[j] = 0.f;
          }
        }
      } else {
        const float nxo = wave_next(o[0], -kInf), nxv = wave_next(v[0], 0.f);
        const float nxm = wave_next(mn[0], 0.f);
#pragma unroll
        for (int j = 0; j < P; ++j) {
          const int u = lane * P + j;
          const float ro = j == P - 1 ? nxo : o[j == P - 1 ? j : j + 1];
          const float rv = j == P - 1 ? nxv : v[j == P - 1 ? j : j + 1];
          const float rm = j == P - 1 ? nxm : mn[j == P - 1 ? j : j + 1];
          // the arc leaving u into beta_{t+1}[u+1]; none leaves position U
          const float to = u < U ? ro : -kInf, tv = wl[j] + rv, tm = rm + vl[j];
          const float bf = wb[j] + v[j], bm = mn[j] + vb[j];
          if constexpr (PH2) {
            el[j] = lt_exp((hh[j].x + to - lpi) + (hh[j].y + tv - lpf));
            kl[j] = el[j] > 0.f ? el[j] * ((hm[j] + tm) - E) : 0.f;
            eb[j] = lt_exp((hh[j].x + o[j] - lpi) + (hh[j].y + bf - lpf));
            kb[j] = eb[j] > 0.f ? eb[j] * ((hm[j] + bm) - E) : 0.f;
          }
          lae_mean(o[j], bf, bm, to, tv, tm, no[j], nv[j], nm[j]);
          if (u > U) {
            no[j] = -kInf;
            nv[j] = 0.f;
            nm[j] = 0.f;
          }
        }
      }
      if constexpr (PH2) {
        const long long rl = obl + (long long)t * U, rb = obb + (long long)t * (U + 1);
#pragma unroll
        for (int j = 0; j < P; ++j) {
          const int u = lane * P + j;
          if (u < U) {
            if (a.em) a.em[rl + u] = el[j];
            if (a.cl) a.cl[rl + u] = kl[j];
          }
          if (u <= U) {
            if (a.bo) a.bo[rb + u] = eb[j];
            if (a.cb) a.cb[rb + u] = kb[j];
          }
        }
      }
#pragma unroll
      for (int j = 0; j < P; ++j) {
        o[j] = no[j];
        v[j] = nv[j];
        mn[j] = nm[j];
      }
    }
  }
}

template <bool BF16, int P, bool HL>
__global__ __launch_bounds__(128) void align_expect_kernel(const XArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char xp_sm[];
  constexpr int SP = 64 * P;  // string positions a wave holds
  constexpr int ES = BF16 ? 2 : 4;
  const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.x;
  const bool rev = __builtin_amdgcn_readfirstlane(tid) >= 64;  // wave R
  const int U = a.U, T = a.T;
  int* ctx = (int*)xp_sm;                  // [SP] context state of position u, times R
  int* yn = ctx + SP;                      // [SP] label class of the arc leaving u
  int* yt = yn + SP;                       // [SP] its true label (0: epsilon)
  float2* mid = (float2*)(yt + SP);        // [2, SP] alpha_m, beta_m
  float* midm = (float*)(mid + 2 * SP);    // [2, SP] abar_m, bbar_m
  unsigned char* region = (unsigned char*)(midm + 2 * SP);  // staged table, then the history
  int* tab = (int*)region;
  int nf = a.nfr[b];
  nf = nf < 0 ? 0 : (nf > T ? T : nf);
  const long long obl = (long long)b * T * U, obb = (long long)b * T * (U + 1);
  const bool keep = a.em || a.bo || a.cl || a.cb;  // else a value-only call

  // ---- rows of padding frames
  for (long long i = (long long)nf * U + tid; i < (long long)T * U; i += 128) {
    if (a.em) a.em[obl + i] = 0.f;
    if (a.cl) a.cl[obl + i] = 0.f;
  }
  for (long long i = (long long)nf * (U + 1) + tid; i < (long long)T * (U + 1); i += 128) {
    if (a.bo) a.bo[obb + i] = 0.f;
    if (a.cb) a.cb[obb + i] = 0.f;
  }

  // ---- string positions: context state and label class
  for (int u = tid; u < SP; u += 128) {
    int y = u < U ? a.labels[(long long)b * U + u] : 0;
    if (y < 0 || y > a.V) y = 0;
    yt[u] = y;
  }
  if (a.stage_tab)
    for (int i = tid; i < a.C * a.V; i += 128) tab[i] = a.table[i];
  __syncthreads();
  if (tid == 0) {
    // positions past U repeat U's state with label class 1: loads in range
    auto walk = [&](const int* tb) {
      int c = 0;
      for (int u = 0; u < SP; ++u) {
        const int y = yt[u];
        ctx[u] = c * a.R;
        yn[u] = y < 1 ? 1 : y;
        if (y != 0) c = tb[c * a.V + y - 1];
      }
    };
    if (a.stage_tab) walk(tab);
    else walk(a.table);
  }
  __syncthreads();
  int ob[P], ol[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    ob[j] = ctx[lane * P + j];
    ol[j] = ob[j] + yn[lane * P + j];
  }
  __syncthreads();  // the table's image is dead: the history may overwrite it

  const long long FRB = (long long)a.C * a.R * ES;
  const unsigned char* wbase = a.W + (long long)b * T * FRB;
  const float* lvb = a.lval + obl;
  const float* bvb = a.bval + obb;
  float* hist;
  if constexpr (HL) hist = (float*)region;
  else hist = a.ws + (long long)b * T * 3 * SP;
  const int nlb = a.nlab[b];
  const int fin = (nlb >= 0 && nlb <= U) ? nlb : -1;
  const int nlc = fin < 0 ? 0 : fin;
  float o[P], v[P], mn[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int u = lane * P + j;
    o[j] = (rev ? u == fin : u == 0) ? 0.f : -kInf;
    v[j] = 0.f;
    mn[j] = 0.f;
  }
  const int m = nf / 2;
  const int n1 = rev ? nf - m : m;  // steps before the midpoint

  // ---- phase 1
  if (!rev)
    exp_phase<BF16, P, false, false>(a, wbase, FRB, lvb, bvb, ob, ol, o, v, mn, hist, obl, obb,
                                     keep, U, nlc, lane, 0, n1, nf, 0.f, 0.f, 0.f);
  else
    exp_phase<BF16, P, true, false>(a, wbase, FRB, lvb, bvb, ob, ol, o, v, mn, hist, obl, obb,
                                    keep, U, nlc, lane, 0, n1, nf, 0.f, 0.f, 0.f);

  // ---- the one meeting of the two waves: log_prob and expected = the
  // posterior mean of abar_m[u] + bbar_m[u], the same in both
  float lpi, lpf, E;
  const bool ok = string_midpoint<P, true>(mid, midm, rev, lane, o, v, mn, lpi, lpf, E);
  if (tid == 0) {
    a.lp[b] = ok ? lpi + lpf : -kInf;
    a.expected[b] = E;
  }
  if (!keep) return;
  if (!ok) {  // unaligned: no path carries weight
    for (long long i = tid; i < (long long)nf * U; i += 128) {
      if (a.em) a.em[obl + i] = 0.f;
      if (a.cl) a.cl[obl + i] = 0.f;
    }
    for (long long i = tid; i < (long long)nf * (U + 1); i += 128) {
      if (a.bo) a.bo[obb + i] = 0.f;
      if (a.cb) a.cb[obb + i] = 0.f;
    }
    return;
  }

  // ---- phase 2
  if (!rev)
    exp_phase<BF16, P, false, true>(a, wbase, FRB, lvb, bvb, ob, ol, o, v, mn, hist, obl, obb,
                                    keep, U, nlc, lane, n1, nf, nf, lpi, lpf, E);
  else
    exp_phase<BF16, P, true, true>(a, wbase, FRB, lvb, bvb, ob, ol, o, v, mn, hist, obl, obb,
                                   keep, U, nlc, lane, n1, nf, nf, lpi, lpf, E);
}

// ---- the dense scatter -------------------------------------------------------
struct SArgs {
  const float* gl;     // [B, T, U]
  const float* gb;     // [B, T, U+1]
  const int* nfr;
  const int* table;
  const int* labels;
  const int* nlab;
  float* dW;           // [B, T, C, V+1]
  int B, T, U, C, V, R;
  int stage_tab;
};

constexpr int kScatFrames = 64;  // frames a workgroup scatters
constexpr int kScatThreads = 256;

// String entry k = 2u + kind (0: the blank arc of position u, 1: its lexical
// arc) adds into dW[t, elem(k)]. Entries that share an element form a chain
// in ascending k; the chain's head sums it in that order and is the only
// writer of the sum: no atomics, bit-equal reruns. The links depend on the
// utterance only: built once per workgroup.
// Zeros. A workgroup is the only writer of its rows [t0, t0 + kScatFrames) of
// utterance b. It first stores zeros over all of them (the stores fly while
// one lane walks the context states), every wave then waits for its own
// stores to be acknowledged (vmcnt(0)) and the workgroup meets at a barrier
// (__syncthreads: a workgroup-scope release / acquire pair): a head's sum to
// an address is issued after every zero to that address has completed, so
// the sum is what memory keeps. No other workgroup touches these rows.
__global__ __launch_bounds__(kScatThreads) void string_scatter_kernel(const SArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sc_sm[];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int U = a.U, S = U + 1, NK = 2 * S;
  int* ctx = (int*)sc_sm;  // [S] context state of position u, times R
  int* yn = ctx + S;       // [S] label class of the arc leaving u
  int* link = yn + S;      // [NK] head << 30 | (next entry + 1)
  int* tab = link + NK;    // the staged table
  int nf = a.nfr[b];
  nf = nf < 0 ? 0 : (nf > a.T ? a.T : nf);
  const long long FR = (long long)a.C * a.R;
  float* dw = a.dW + (long long)b * a.T * FR;
  const int t0 = blockIdx.x * kScatFrames;
  const int tz = t0 + kScatFrames < a.T ? t0 + kScatFrames : a.T;
  zero_rows(dw + (long long)t0 * FR, (long long)(tz - t0) * FR, tid, kScatThreads);
  const int t1 = tz < nf ? tz : nf;
  if (t0 >= t1) return;  // workgroup-uniform: padding frames stay zero
  int nl = a.nlab[b];
  nl = nl < 0 ? 0 : (nl > U ? U : nl);
  if (a.stage_tab)
    for (int i = tid; i < a.C * a.V; i += kScatThreads) tab[i] = a.table[i];
  __syncthreads();
  if (tid == 0) {
    const int* tb = a.stage_tab ? tab : a.table;
    int c = 0;
    for (int u = 0; u < S; ++u) {
      int y = u < U ? a.labels[(long long)b * U + u] : 0;
      if (y < 0 || y > a.V) y = 0;
      ctx[u] = c * a.R;
      yn[u] = y < 1 ? 1 : y;  // an epsilon reads label 1's weight
      if (y != 0) c = tb[c * a.V + y - 1];
    }
  }
  __syncthreads();
  auto elem = [&](int k) {  // W element of string entry k, or -1: positions past num_labels
    const int u = k >> 1;
    return (k & 1) == 0 ? (u <= nl ? ctx[u] : -1) : (u < nl ? ctx[u] + yn[u] : -1);
  };
  for (int k = tid; k < NK; k += kScatThreads) {
    const int e = elem(k);
    int head = e >= 0 ? 1 : 0, nxt = -1;
    if (e >= 0)
      for (int k2 = 0; k2 < NK; ++k2) {
        if (elem(k2) != e) continue;
        if (k2 < k) head = 0;
        else if (k2 > k && nxt < 0) nxt = k2;
      }
    link[k] = (head << 30) | (nxt + 1);
  }
  wait_vmcnt(0);    // this wave's zeros are in memory ...
  __syncthreads();  // ... and so are every other wave's: the sums may follow
  const float* gl = a.gl + (long long)b * a.T * U;
  const float* gb = a.gb + (long long)b * a.T * S;
  for (int i = tid; i < (t1 - t0) * NK; i += kScatThreads) {
    const int t = t0 + i / NK, k = i % NK;
    if (!(link[k] >> 30)) continue;
    float s = 0.f;
    for (int kk = k; kk >= 0; kk = (link[kk] & 0x3fffffff) - 1)
      s += (kk & 1) ? gl[(long long)t * U + (kk >> 1)] : gb[(long long)t * S + (kk >> 1)];
    dw[(long long)t * FR + elem(k)] = s;
  }
}

// The refusals both entry points make (flags: how the entry looks at the dtype).
int string_check(const char* entry, const lt_graph* g, const lt_table_problem* pb, int flags) {
  return table_check(entry, g, pb, kChkString | flags, [&] {
    if (g->expansions > 0)
      return fail(LT_EUNSUPPORTED,
                  std::string(entry) + ": FrameLabelDependent (expansions >= 1)");
    if (pb->max_labels > 255)
      return fail(LT_EUNSUPPORTED, std::string(entry) + ": max_labels > 255");
    return LT_OK;
  });
}

// Validates the shape and lays out LDS / workspace.
int exp_plan(const lt_graph* g, const lt_table_problem* pb, StringPlan* pl) {
  if (int rc = string_check("lt_table_align_expectation", g, pb, kChkDtypeLast)) return rc;
  pl->P = string_positions(pb->max_labels);
  const long long SP = 64LL * pl->P;
  // ctx, yn, yt; the two midpoint triples; a frame of history is a triple a position
  string_layout(g, pb, 3 * 4 * SP + 2 * 12 * SP, 12 * SP, 0, pl);
  return LT_OK;
}

}  // namespace

extern "C" {

int lt_table_align_expectation_workspace_bytes(const lt_graph* g, const lt_table_problem* pb,
                                               size_t* bytes) {
  StringPlan pl;
  if (int rc = exp_plan(g, pb, &pl)) return rc;
  if (bytes) *bytes = pl.ws;
  return LT_OK;
}

int lt_table_align_expectation(const lt_graph* g, const lt_table_problem* pb, const void* W,
                               const float* lexical_values, const float* blank_values,
                               const int32_t* num_frames, const int32_t* labels,
                               const int32_t* num_labels, float* expected, float* log_prob,
                               float* emission, float* blank_occ, float* cov_lex,
                               float* cov_blank, void* workspace, size_t workspace_bytes,
                               void* stream) {
  StringPlan pl;
  if (int rc = exp_plan(g, pb, &pl)) return rc;
  if (pb->batch == 0) return LT_OK;
  const bool frames = pb->max_frames > 0;
  const bool keep = emission || blank_occ || cov_lex || cov_blank;
  if ((!W && frames) || !num_frames || !num_labels || !expected || !log_prob ||
      (!lexical_values && frames && pb->max_labels > 0) || (!blank_values && frames) ||
      (pb->max_labels > 0 && !labels))
    return fail(LT_EINVAL, "null pointer");
  const bool bf16 = pb->weight_dtype == LT_DTYPE_BF16;
  if (((uintptr_t)W & (bf16 ? 1 : 3)) || ((uintptr_t)lexical_values & 3) ||
      ((uintptr_t)blank_values & 3) || ((uintptr_t)num_frames & 3) || ((uintptr_t)labels & 3) ||
      ((uintptr_t)num_labels & 3) || ((uintptr_t)expected & 3) || ((uintptr_t)log_prob & 3) ||
      ((uintptr_t)emission & 3) || ((uintptr_t)blank_occ & 3) || ((uintptr_t)cov_lex & 3) ||
      ((uintptr_t)cov_blank & 3) || ((uintptr_t)workspace & 7))
    return fail(LT_EINVAL, "misaligned pointer");
  // a value-only call keeps no history
  if (keep && pl.ws && (!workspace || workspace_bytes < pl.ws))
    return fail(LT_EINVAL, "workspace too small");
  XArgs a;
  memset(&a, 0, sizeof(a));
  a.W = (const unsigned char*)W;
  a.lval = lexical_values;
  a.bval = blank_values;
  a.nfr = num_frames;
  a.table = g->next_state;
  a.labels = labels;
  a.nlab = num_labels;
  a.expected = expected;
  a.lp = log_prob;
  a.em = emission;
  a.bo = blank_occ;
  a.cl = cov_lex;
  a.cb = cov_blank;
  a.ws = (float*)workspace;
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
    auto k = pl.hist_lds ? align_expect_kernel<BF16, P, true> : align_expect_kernel<BF16, P, false>;
    return launch(k, dim3(a.B), dim3(128), pl.lds, st, a, "alignment expectation");
  });
}

int lt_table_string_scatter(const lt_graph* g, const lt_table_problem* pb, const float* g_lex,
                            const float* g_blank, const int32_t* num_frames,
                            const int32_t* labels, const int32_t* num_labels, float* dW,
                            void* stream) {
  if (int rc = string_check("lt_table_string_scatter", g, pb, kChkNoDtype)) return rc;
  if (pb->batch == 0 || pb->max_frames == 0) return LT_OK;
  if (!num_frames || !num_labels || !dW || !g_blank || (pb->max_labels > 0 && (!labels || !g_lex)))
    return fail(LT_EINVAL, "null pointer");
  if (((uintptr_t)g_lex & 3) || ((uintptr_t)g_blank & 3) || ((uintptr_t)num_frames & 3) ||
      ((uintptr_t)labels & 3) || ((uintptr_t)num_labels & 3) || ((uintptr_t)dW & 3))
    return fail(LT_EINVAL, "misaligned pointer");
  SArgs a;
  memset(&a, 0, sizeof(a));
  a.gl = g_lex;
  a.gb = g_blank;
  a.nfr = num_frames;
  a.table = g->next_state;
  a.labels = labels;
  a.nlab = num_labels;
  a.dW = dW;
  a.B = pb->batch;
  a.T = pb->max_frames;
  a.U = pb->max_labels;
  a.C = g->num_states;
  a.V = g->vocab_size;
  a.R = g->vocab_size + 1;
  const long long tabb = stage_table(g);
  a.stage_tab = tabb ? 1 : 0;
  const int S = a.U + 1;
  const int lds = 4 * (2 * S + 2 * S) + (int)tabb;
  const int chunks = (a.T + kScatFrames - 1) / kScatFrames;
  return launch(string_scatter_kernel, dim3(chunks, a.B), dim3(kScatThreads), lds,
                (hipStream_t)stream, a, "string scatter");
}

}  // extern "C"
