// lt_align_expect_long.hip -- the alignment expectation of lt_align_expect.hip
// and its dense scatter for label strings of 256 <= U <= 1023
// (include/lt_string_expect_long.h): the same definition, the same (integer
// part, fraction) log values and conditional means per position (lae_mean,
// expect_step below), the string split over several waves.
//
// lt_table_align_expectation_long: ONE launch, one workgroup per utterance,
// two directions of NW = ceil((U+1)/256) waves each (NW in {2, 3, 4}: 256 to
// 512 threads). Wave w of a direction holds positions 256w .. 256w+255, four
// consecutive ones a lane. Direction F runs (alpha, abar) upward from frame 0,
// direction R (beta, bbar) downward from frame nf-1; they meet once, at
// m = nf/2, and each emits the half of the frames it enters with its own
// vectors in registers -- lt_align_expect.hip's plan.
//
//   carry      Inside a wave position u-1 (F) / u+1 (R) is one lane shift
//              away. Across a wave boundary the carry is a TRIPLE: F's wave w
//              needs, at frame t, alpha_t[256w-1] + lex_t[256w-1] as (integer
//              part, fraction) and abar_t[256w-1] + lv_t[256w-1] -- lane 63's
//              last lexical term of wave w-1 at the same frame; R's wave w
//              needs (beta_{t+1}, bbar_{t+1})[256(w+1)], lane 0's first term of
//              wave w+1. The triple is the fill value of the receiving wave's
//              three shifts (expect_step's fo, fv, fm).
//   pipeline   lt_align_post_long.hip's: frames in blocks of kXlF; at
//              block-step s the wave of rank r (F: r = w, R: r = NW-1-w) runs
//              block s-r of its direction, writes the block's outgoing carries
//              into an LDS ring [direction][NW-1][2][kXlF] of float4 (x, y, z:
//              the triple; double-buffered by block parity) and its neighbour
//              reads them one block-step later: ONE __syncthreads() per
//              block-step, none per frame. The step count is the same in all
//              2 NW waves (computed from nf alone); a wave with no block at a
//              step only passes the barrier. A block's incoming carries are
//              read once, frame f in lane f, and handed out by v_readlane.
//   phase 1    F stores (alpha_t, abar_t) for t < m, R stores (beta_{t+1},
//              bbar_{t+1}) for t >= m into the history [T, 3, 256 NW] in the
//              caller's workspace: per row 256 NW (integer part, fraction)
//              pairs, then 256 NW means. A value-only call stores nothing.
//   midpoint   Every wave publishes its slice of (alpha_m, abar_m) or (beta_m,
//              bbar_m) in LDS, one barrier, then every wave reduces all 256 NW
//              positions from the same LDS words by the same instructions:
//              log_prob and expected are bit-equal in all waves, the unaligned
//              exit is workgroup-uniform, expected is known before phase 2.
//   phase 2    The pipeline refills. Each wave reads the other direction's
//              history row at its own columns. F needs beta_{t+1} at u (blank
//              arc) and u+1 (lexical arc): the fifth column of a lane is the
//              next lane's first (one DPP shift per component), and lane 63
//              alone loads column 256(w+1) from the row -- it is in the
//              workspace, so that shift needs no carry. Each wave stores its
//              256 columns of the frame's rows of the non-NULL arrays.
// Weights, both value rows and history rows run kD frames ahead through
// register rings across the blocks: no load sits on the recursion chain. A
// term of weight -inf is selected out, never multiplied. No atomics.
//
// lt_table_string_scatter_long: lt_table_string_scatter's rule with the chains
// found by a sort. A workgroup owns kScatFrames rows of one utterance's dW,
// zeroes them, sorts the keys (element << 11 | k) of the 2(U+1) string entries
// in LDS (bitonic, 64-bit keys: a frame may hold up to 2^31 elements) -- runs
// of equal element are the chains, in ascending k -- and behind vmcnt(0) and a
// workgroup barrier each run's first entry writes the run's sum.
#include "lt_string_common.h"

namespace {

constexpr int kXlF = 16;  // frames of a pipeline block (tests/test_gpu_align_expect_long.py: F)

struct XlArgs {
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
  float* ws;           // history [B, T, 3, 256 NW]
  int B, T, U, C, V, R;
  int stage_tab;       // the next-state table is staged in LDS for the walk
};

LT_DEVINL float lane_value(float x, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l));
}

// lt_align_expect.hip's lae_mean, term for term (that file keeps it in its own
// unnamed namespace, and its kernels' code is pinned by their rerun tests):
// lae_split with the conditional means of its two terms. The result's mean is
// the softmax-weighted mean of ma and mb; a zero term (-inf, or underflowed)
// is selected out: its mean is not read into the arithmetic. Both zero, or a
// result that is not finite: mean 0.
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
  const float mix = e > 0.f ? __builtin_fmaf(m2 - m1, e * __builtin_amdgcn_rcpf(s), m1) : m1;
  mo = (zero || !fin) ? 0.f : mix;
}

// The frame's rows of the four outputs (each nullable), already at the utterance.
struct XlRows {
  float *em, *bo, *cl, *cb;
};

// One frame of the two recursions for a lane's four consecutive positions from
// u0 -- the frame step of lt_align_expect.hip's exp_phase with the lane's first
// position and the shifts' fill values as arguments. (o, v, mn) is (alpha_t,
// abar_t) (!REV) or (beta_{t+1}, bbar_{t+1}) (REV); wb / wl the frame's blank /
// lexical weights, vb / vl its blank / lexical values; the step leaves
// (alpha_{t+1}, abar_{t+1}) / (beta_t, bbar_t). (fo, fv, fm) is what the wave
// shift hands the lane with no neighbour: F's lane 0 the lexical term of
// position u0-1, R's lane 63 (beta_{t+1}, bbar_{t+1})[u0+4] -- (-inf, 0, 0)
// where the string ends there, the neighbouring wave's carry where it goes on.
// PH2: (hh, hm) is the other direction's history at the lane's own columns and
// the frame, (xh, xm) in lane 63 of F its column u0+4 (the fill of F's
// history shift); the frame's rows get their columns u < U (lexical) and
// u <= U (blank).
template <bool REV, bool PH2>
LT_DEVINL void expect_step(float (&o)[4], float (&v)[4], float (&mn)[4], const float (&wb)[4],
                           const float (&wl)[4], const float (&vb)[4], const float (&vl)[4],
                           const float2 (&hh)[4], const float (&hm)[4], float2 xh, float xm,
                           const XlRows& rows, long long rl, long long rb, int U, int u0, float fo,
                           float fv, float fm, float lpi, float lpf, float E) {
  constexpr int P = 4;
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
      // beta_{t+1}[u+1]: the row's next column
      const float nxo = wave_next(hh[0].x, xh.x), nxf = wave_next(hh[0].y, xh.y);
      const float nxm = wave_next(hm[0], xm);
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
    const float po = wave_prev(o[P - 1], fo), pf = wave_prev(lf[P - 1], fv);
    const float pq = wave_prev(lm[P - 1], fm);
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const int u = u0 + j;
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
    const float nxo = wave_next(o[0], fo), nxv = wave_next(v[0], fv);
    const float nxm = wave_next(mn[0], fm);
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const int u = u0 + j;
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
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const int u = u0 + j;
      if (u < U) {
        if (rows.em) rows.em[rl + u] = el[j];
        if (rows.cl) rows.cl[rl + u] = kl[j];
      }
      if (u <= U) {
        if (rows.bo) rows.bo[rb + u] = eb[j];
        if (rows.cb) rows.cb[rb + u] = kb[j];
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

// One phase of wave w of a direction: steps i0..i1-1 (step i is frame t = i
// (F) or nf-1-i (R)) in blocks of kXlF, block k at block-step k + rank, and
// `nsteps` barriers whatever the wave has to do. ring: the direction's
// [NW-1][2][kXlF] carries; edge e is written by rank e and read by rank e+1.
template <bool BF16, int NW, bool REV, bool PH2>
LT_DEVINL void xl_phase(const unsigned char* wbase, long long frame_bytes, const float* lvb,
                        const float* bvb, const int (&ob)[4], const int (&ol)[4], float (&o)[4],
                        float (&v)[4], float (&mn)[4], float* hist, const XlRows& rows, bool keep,
                        int U, int nlc, int lane, int w, int i0, int i1, int nf, int nsteps,
                        float4* ring, float lpi, float lpf, float E) {
  constexpr int P = 4, SPT = 256 * NW, F = kXlF;
  // frames of weights / values / history in flight; F is a multiple. Phase 2
  // carries the history beside them: half the depth keeps the rings in registers
  constexpr int D = PH2 ? 4 : 8;
  static_assert(F % D == 0, "a block is whole rounds of the register ring");
  const int rank = REV ? NW - 1 - w : w;
  const int u0 = 256 * w + lane * P;
  const bool has_in = rank > 0, has_out = rank < NW - 1;
  const float4* rin = ring + (has_in ? rank - 1 : 0) * 2 * F;
  float4* rout = ring + (has_out ? rank : 0) * 2 * F;
  // value columns this lane reads: lexical u < nl, blank u <= nl (others: 0, not read)
  bool hl[P], hb[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    hl[j] = u0 + j < nlc;
    hb[j] = u0 + j <= nlc;
  }
  // F's lane 63 reads column 256(w+1) of R's row: the next wave's first (the
  // last wave has none: position 256 NW is never a live arc's end)
  const bool x5 = PH2 && !REV && lane == 63 && w < NW - 1;
  float pb[D][P], pl[D][P], qb[D][P], ql[D][P], pm[D][P], pxm[D];
  float2 ph[D][P], px[D];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    px[d] = make_float2(-kInf, 0.f);
    pxm[d] = 0.f;
  }
  auto fetch = [&](int d, int t) {
    const unsigned char* wf = wbase + (long long)t * frame_bytes;
    const float* lf = lvb + (long long)t * U;
    const float* bf = bvb + (long long)t * (U + 1);
    const float* hr = hist + (long long)t * 3 * SPT;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const int u = u0 + j;
      pb[d][j] = ldw<BF16>(wf, ob[j]);
      pl[d][j] = ldw<BF16>(wf, ol[j]);
      qb[d][j] = hb[j] ? bf[u] : 0.f;
      ql[d][j] = hl[j] ? lf[u] : 0.f;
      if constexpr (PH2) {
        ph[d][j] = ((const float2*)hr)[u];
        pm[d][j] = hr[2 * SPT + u];
      }
    }
    if constexpr (PH2 && !REV) {
      if (x5) {
        px[d] = ((const float2*)hr)[u0 + P];
        pxm[d] = hr[2 * SPT + u0 + P];
      }
    }
  };
  if (i0 < i1) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int i = i0 + d < i1 ? i0 + d : i1 - 1;
      fetch(d, REV ? nf - 1 - i : i);
    }
  }
  for (int s = 0; s < nsteps; ++s) {
    const int k = s - rank;
    const int ib = i0 + k * F;
    if (k >= 0 && ib < i1) {
      // the block's incoming carries, frame f in lane f
      float4 cin = make_float4(-kInf, 0.f, 0.f, 0.f);
      if (has_in && lane < F) cin = rin[(k & 1) * F + lane];
      float4* co = rout + (k & 1) * F;
      for (int h = 0; h < F; h += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
          const int f = h + d, i = ib + f;
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
          const float2 xh = px[d];
          const float xm = pxm[d];
          {
            const int in = i + D < i1 ? i + D : i1 - 1;
            fetch(d, REV ? nf - 1 - in : in);
          }
          if constexpr (!PH2) {
            if (keep) {
              float* hr = hist + (long long)t * 3 * SPT;
#pragma unroll
              for (int j = 0; j < P; ++j) {
                ((float2*)hr)[u0 + j] = make_float2(o[j], v[j]);
                hr[2 * SPT + u0 + j] = mn[j];
              }
            }
          }
          // what the next wave's shifts take in at this frame
          if (has_out && lane == (REV ? 0 : 63))
            co[f] = REV ? make_float4(o[0], v[0], mn[0], 0.f)
                        : make_float4(o[P - 1], v[P - 1] + wl[P - 1], mn[P - 1] + vl[P - 1], 0.f);
          const float fo = lane_value(cin.x, f), fv = lane_value(cin.y, f);
          const float fm = lane_value(cin.z, f);
          expect_step<REV, PH2>(o, v, mn, wb, wl, vb, vl, hh, hm, xh, xm, rows, (long long)t * U,
                                (long long)t * (U + 1), U, u0, fo, fv, fm, lpi, lpf, E);
        }
      }
    }
    __syncthreads();  // the block's carries
  }
}

// The one meeting of the 2 NW waves: each publishes its 256 positions of
// (alpha_m, abar_m) (F) or (beta_m, bbar_m) (R) in mid / midm [2, 256 NW], ONE
// barrier, then every wave computes log_prob = lpi + lpf = logsumexp_u(alpha_m[u]
// + beta_m[u]) and E, the posterior mean of abar_m[u] + bbar_m[u], over all
// positions (lane l: the four from 256k + 4l of every slice k) from the same
// LDS words by the same instructions: bit-equal in all waves. Returns whether
// any path carries weight (the same in all waves); lpi = 0, E = 0 when none does.
template <int NW>
LT_DEVINL bool xl_midpoint(float2* mid, float* midm, bool rev, int w, int lane,
                           const float (&o)[4], const float (&v)[4], const float (&mn)[4],
                           float& lpi, float& lpf, float& E) {
  constexpr int SPT = 256 * NW, N = 4 * NW;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    mid[(rev ? SPT : 0) + 256 * w + lane * 4 + j] = make_float2(o[j], v[j]);
    midm[(rev ? SPT : 0) + 256 * w + lane * 4 + j] = mn[j];
  }
  __syncthreads();  // history rows and the midpoint vectors
  float si[N], sf[N], sm[N];
  float mx = -kInf;
#pragma unroll
  for (int n = 0; n < N; ++n) {
    const int u = 256 * (n / 4) + lane * 4 + n % 4;
    const float2 x = mid[u], y = mid[SPT + u];
    si[n] = x.x + y.x;
    sf[n] = x.y + y.y;
    sm[n] = midm[u] + midm[SPT + u];
    mx = fmaxf(mx, si[n] + sf[n]);
  }
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) mx = fmaxf(mx, __shfl_xor(mx, s, 64));
  const bool ok = __builtin_isfinite(mx);
  lpi = ok ? floorf(mx) : 0.f;
  float sum = 0.f, ex = 0.f;
#pragma unroll
  for (int n = 0; n < N; ++n) {
    const float e = lt_exp((si[n] - lpi) + sf[n]);
    sum += e;
    ex += e > 0.f ? e * sm[n] : 0.f;
  }
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    sum += __shfl_xor(sum, s, 64);
    ex += __shfl_xor(ex, s, 64);
  }
  lpf = lt_log_acc(sum);
  E = ok ? ex / sum : 0.f;
  return ok;
}

template <bool BF16, int NW>
__global__ __launch_bounds__(128 * NW) void align_expect_long_kernel(const XlArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char xl_sm[];
  constexpr int P = 4, SPT = 256 * NW, NT = 128 * NW, F = kXlF;
  constexpr int ES = BF16 ? 2 : 4;
  const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.x;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool rev = wid >= NW;  // direction R
  const int w = rev ? wid - NW : wid;
  const int U = a.U, T = a.T;
  int nf = a.nfr[b];
  nf = nf < 0 ? 0 : (nf > T ? T : nf);
  const long long obl = (long long)b * T * U, obb = (long long)b * T * (U + 1);
  const bool keep = a.em || a.bo || a.cl || a.cb;  // else a value-only call
  XlRows rows;
  rows.em = a.em ? a.em + obl : nullptr;
  rows.cl = a.cl ? a.cl + obl : nullptr;
  rows.bo = a.bo ? a.bo + obb : nullptr;
  rows.cb = a.cb ? a.cb + obb : nullptr;

  // ---- rows of padding frames
  for (long long i = (long long)nf * U + tid; i < (long long)T * U; i += NT) {
    if (rows.em) rows.em[i] = 0.f;
    if (rows.cl) rows.cl[i] = 0.f;
  }
  for (long long i = (long long)nf * (U + 1) + tid; i < (long long)T * (U + 1); i += NT) {
    if (rows.bo) rows.bo[i] = 0.f;
    if (rows.cb) rows.cb[i] = 0.f;
  }

  // ---- string positions: context state and label class
  int ob[P], ol[P];
  const StringLds sl = string_prologue<P, NT, 24, SPT>(a, b, tid, lane, xl_sm, ob, ol, 256 * w);
  float2* mid = (float2*)sl.mid;            // [2, SPT] alpha_m, beta_m
  float* midm = (float*)(mid + 2 * SPT);    // [2, SPT] abar_m, bbar_m
  // the carry ring takes the staged table's place
  float4* ring = (float4*)sl.region + (rev ? (NW - 1) * 2 * F : 0);

  const long long FRB = (long long)a.C * a.R * ES;
  const unsigned char* wbase = a.W + (long long)b * T * FRB;
  const float* lvb = a.lval + obl;
  const float* bvb = a.bval + obb;
  float* hist = keep ? a.ws + (long long)b * T * 3 * SPT : nullptr;
  const int nlb = a.nlab[b];
  const int fin = (nlb >= 0 && nlb <= U) ? nlb : -1;
  const int nlc = fin < 0 ? 0 : fin;
  float o[P], v[P], mn[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int u = 256 * w + lane * P + j;
    o[j] = (rev ? u == fin : u == 0) ? 0.f : -kInf;
    v[j] = 0.f;
    mn[j] = 0.f;
  }
  const int m = nf / 2;
  const int n1 = rev ? nf - m : m;  // steps before the midpoint
  // block-steps of a phase: the longer half's blocks (nf - m >= m) and the skew
  const int nb = (nf - m + F - 1) / F;
  const int nsteps = nb ? nb + NW - 1 : 0;

  // ---- phase 1
  if (!rev)
    xl_phase<BF16, NW, false, false>(wbase, FRB, lvb, bvb, ob, ol, o, v, mn, hist, rows, keep, U,
                                     nlc, lane, w, 0, n1, nf, nsteps, ring, 0.f, 0.f, 0.f);
  else
    xl_phase<BF16, NW, true, false>(wbase, FRB, lvb, bvb, ob, ol, o, v, mn, hist, rows, keep, U,
                                    nlc, lane, w, 0, n1, nf, nsteps, ring, 0.f, 0.f, 0.f);

  // ---- the one meeting of all waves: log_prob and expected, the same in each
  float lpi, lpf, E;
  const bool ok = xl_midpoint<NW>(mid, midm, rev, w, lane, o, v, mn, lpi, lpf, E);
  if (tid == 0) {
    a.lp[b] = ok ? lpi + lpf : -kInf;
    a.expected[b] = E;
  }
  if (!keep) return;
  if (!ok) {  // unaligned: no path carries weight
    for (long long i = tid; i < (long long)nf * U; i += NT) {
      if (rows.em) rows.em[i] = 0.f;
      if (rows.cl) rows.cl[i] = 0.f;
    }
    for (long long i = tid; i < (long long)nf * (U + 1); i += NT) {
      if (rows.bo) rows.bo[i] = 0.f;
      if (rows.cb) rows.cb[i] = 0.f;
    }
    return;
  }

  // ---- phase 2
  if (!rev)
    xl_phase<BF16, NW, false, true>(wbase, FRB, lvb, bvb, ob, ol, o, v, mn, hist, rows, keep, U,
                                    nlc, lane, w, n1, nf, nf, nsteps, ring, lpi, lpf, E);
  else
    xl_phase<BF16, NW, true, true>(wbase, FRB, lvb, bvb, ob, ol, o, v, mn, hist, rows, keep, U,
                                   nlc, lane, w, n1, nf, nf, nsteps, ring, lpi, lpf, E);
}

// ---- the dense scatter -------------------------------------------------------
struct SlArgs {
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
constexpr int kKeyBits = 11;     // k = 2u + kind < 2048

// String entry k = 2u + kind (0: the blank arc of position u, 1: its lexical
// arc) adds into dW[t, elem(k)]. The entries are sorted by (elem, k): a run of
// equal elem is a chain in ascending k, its first entry sums it in that order
// and is the only writer of the sum: no atomics, bit-equal reruns. The order
// depends on the utterance only: sorted once per workgroup.
// Zeros. A workgroup is the only writer of its rows [t0, t0 + kScatFrames) of
// utterance b. It first stores zeros over all of them (the stores fly while
// one lane walks the context states and the workgroup sorts), every wave then
// waits for its own stores to be acknowledged (vmcnt(0)) and the workgroup
// meets at a barrier: a sum to an address is issued after every zero to that
// address has completed, so the sum is what memory keeps.
__global__ __launch_bounds__(kScatThreads) void string_scatter_long_kernel(const SlArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sl_sm[];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int U = a.U, S = U + 1, NK = 2 * S;
  const int N = NK <= 1024 ? 1024 : 2048;  // keys sorted: a power of two >= NK
  unsigned long long* key = (unsigned long long*)sl_sm;  // [N] elem << 11 | k; ~0: no element
  int* ctx = (int*)(key + N);  // [S] context state of position u, times R
  int* yn = ctx + S;           // [S] label class of the arc leaving u
  int* tab = yn + S;           // the staged table
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
  for (int k = tid; k < N; k += kScatThreads) {
    const int u = k >> 1;
    // W element of string entry k, or none: positions past num_labels, the padding keys
    long long e = -1;
    if (k < NK) e = (k & 1) == 0 ? (u <= nl ? ctx[u] : -1) : (u < nl ? ctx[u] + yn[u] : -1);
    key[k] = e < 0 ? ~0ull : ((unsigned long long)e << kKeyBits) | (unsigned)k;
  }
  __syncthreads();
  // bitonic sort, ascending
  for (int kk = 2; kk <= N; kk <<= 1)
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < N; i += kScatThreads) {
        const int x = i ^ j;
        if (x > i) {
          const unsigned long long p = key[i], q = key[x];
          if ((p > q) == ((i & kk) == 0)) {
            key[i] = q;
            key[x] = p;
          }
        }
      }
      __syncthreads();
    }
  wait_vmcnt(0);    // this wave's zeros are in memory ...
  __syncthreads();  // ... and so are every other wave's: the sums may follow
  const float* gl = a.gl + (long long)b * a.T * U;
  const float* gb = a.gb + (long long)b * a.T * S;
  for (int i = tid; i < (t1 - t0) * N; i += kScatThreads) {
    const int t = t0 + i / N, r = i % N;
    const unsigned long long q = key[r];
    if (q == ~0ull) continue;
    const unsigned long long e = q >> kKeyBits;
    if (r > 0 && (key[r - 1] >> kKeyBits) == e) continue;  // not its run's first
    float s = 0.f;
    for (int rr = r; rr < N; ++rr) {
      const unsigned long long qq = key[rr];
      if ((qq >> kKeyBits) != e) break;  // ~0 >> 11 is no element either
      const int k = (int)(qq & ((1u << kKeyBits) - 1));
      s += (k & 1) ? gl[(long long)t * U + (k >> 1)] : gb[(long long)t * S + (k >> 1)];
    }
    dw[(long long)t * FR + (long long)e] = s;
  }
}

// The refusals all entry points here make (flags: how the entry looks at the dtype).
int long_check(const char* entry, const lt_graph* g, const lt_table_problem* pb, int flags) {
  return table_check(entry, g, pb, kChkString | flags, [&] {
    if (g->expansions > 0)
      return fail(LT_EUNSUPPORTED,
                  std::string(entry) + ": FrameLabelDependent (expansions >= 1)");
    if (pb->max_labels < 256 || pb->max_labels > 1023)
      return fail(LT_EUNSUPPORTED, std::string(entry) + ": max_labels outside 256..1023");
    return LT_OK;
  });
}

struct XlPlan {
  int NW, stage_tab, lds;
  size_t ws;
};

// Validates the shape and lays out LDS / workspace.
int xl_plan(const lt_graph* g, const lt_table_problem* pb, XlPlan* pl) {
  if (int rc = long_check("lt_table_align_expectation_long", g, pb, kChkDtypeLast)) return rc;
  pl->NW = (pb->max_labels + 256) / 256;
  const long long SPT = 256LL * pl->NW;
  const long long stage = stage_table(g);
  pl->stage_tab = stage ? 1 : 0;
  // ctx, yn, yt; the two midpoint triples; then the staged table, and in its place the carry ring
  const long long ringb = 2LL * (pl->NW - 1) * 2 * kXlF * 16;
  const long long lds = (3 * 4 + 2 * 12) * SPT + ((std::max(stage, ringb) + 15) & ~15LL);
  if (lds > kTabLds)
    return fail(LT_EUNSUPPORTED, "lt_table_align_expectation_long: the LDS layout does not fit");
  pl->lds = (int)lds;
  // a frame of history is (integer part, fraction, mean) a position
  pl->ws = (size_t)(((long long)pb->batch * pb->max_frames * SPT * 12 + 255) & ~255LL);
  return LT_OK;
}

}  // namespace

extern "C" {

int lt_table_align_expectation_long_workspace_bytes(const lt_graph* g, const lt_table_problem* pb,
                                                    size_t* bytes) {
  XlPlan pl;
  if (int rc = xl_plan(g, pb, &pl)) return rc;
  if (bytes) *bytes = pl.ws;
  return LT_OK;
}

int lt_table_align_expectation_long(const lt_graph* g, const lt_table_problem* pb, const void* W,
                                    const float* lexical_values, const float* blank_values,
                                    const int32_t* num_frames, const int32_t* labels,
                                    const int32_t* num_labels, float* expected, float* log_prob,
                                    float* emission, float* blank_occ, float* cov_lex,
                                    float* cov_blank, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  XlPlan pl;
  if (int rc = xl_plan(g, pb, &pl)) return rc;
  if (pb->batch == 0) return LT_OK;
  const bool frames = pb->max_frames > 0;
  const bool keep = emission || blank_occ || cov_lex || cov_blank;
  if ((!W && frames) || !num_frames || !num_labels || !expected || !log_prob ||
      (!lexical_values && frames) || (!blank_values && frames) || !labels)
    return fail(LT_EINVAL, "null pointer");
  // a value-only call keeps no history
  if (keep && pl.ws && (!workspace || workspace_bytes < pl.ws))
    return fail(LT_EINVAL, "workspace too small");
  const bool bf16 = pb->weight_dtype == LT_DTYPE_BF16;
  if (((uintptr_t)W & (bf16 ? 1 : 3)) || ((uintptr_t)lexical_values & 3) ||
      ((uintptr_t)blank_values & 3) || ((uintptr_t)num_frames & 3) || ((uintptr_t)labels & 3) ||
      ((uintptr_t)num_labels & 3) || ((uintptr_t)expected & 3) || ((uintptr_t)log_prob & 3) ||
      ((uintptr_t)emission & 3) || ((uintptr_t)blank_occ & 3) || ((uintptr_t)cov_lex & 3) ||
      ((uintptr_t)cov_blank & 3) || ((uintptr_t)workspace & 7))
    return fail(LT_EINVAL, "misaligned pointer");
  XlArgs a;
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
  a.ws = keep ? (float*)workspace : nullptr;
  a.B = pb->batch;
  a.T = pb->max_frames;
  a.U = pb->max_labels;
  a.C = g->num_states;
  a.V = g->vocab_size;
  a.R = g->vocab_size + 1;
  a.stage_tab = pl.stage_tab;
  hipStream_t st = (hipStream_t)stream;
  return dispatch(bf16, [&](auto bf) {
    constexpr bool BF16 = decltype(bf)::value;
    auto k = pl.NW == 2   ? align_expect_long_kernel<BF16, 2>
             : pl.NW == 3 ? align_expect_long_kernel<BF16, 3>
                          : align_expect_long_kernel<BF16, 4>;
    return launch(k, dim3(a.B), dim3(128 * pl.NW), pl.lds, st, a, "long alignment expectation");
  });
}

int lt_table_string_scatter_long(const lt_graph* g, const lt_table_problem* pb, const float* g_lex,
                                 const float* g_blank, const int32_t* num_frames,
                                 const int32_t* labels, const int32_t* num_labels, float* dW,
                                 void* stream) {
  if (int rc = long_check("lt_table_string_scatter_long", g, pb, kChkNoDtype)) return rc;
  if (pb->batch == 0 || pb->max_frames == 0) return LT_OK;
  if (!num_frames || !num_labels || !dW || !g_blank || !labels || !g_lex)
    return fail(LT_EINVAL, "null pointer");
  if (((uintptr_t)g_lex & 3) || ((uintptr_t)g_blank & 3) || ((uintptr_t)num_frames & 3) ||
      ((uintptr_t)labels & 3) || ((uintptr_t)num_labels & 3) || ((uintptr_t)dW & 3))
    return fail(LT_EINVAL, "misaligned pointer");
  SlArgs a;
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
  const int N = 2 * S <= 1024 ? 1024 : 2048;
  const int lds = 8 * N + 4 * 2 * S + (int)tabb;
  const int chunks = (a.T + kScatFrames - 1) / kScatFrames;
  return launch(string_scatter_long_kernel, dim3(chunks, a.B), dim3(kScatThreads), lds,
                (hipStream_t)stream, a, "long string scatter");
}

}  // extern "C"
