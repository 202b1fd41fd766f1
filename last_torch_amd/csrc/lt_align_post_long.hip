// lt_align_post_long.hip -- the emission posteriors of lt_align_post.hip for
// label strings of 256 <= U <= 1023 (include/lt_posterior_long.h): the same
// definition, the same (integer part, fraction) arithmetic per position
// (post_step below), the string split over several waves.
//
// One workgroup per utterance, two directions of NW = ceil((U+1)/256) waves
// each (NW in {2, 3, 4}: 256 to 512 threads). Wave w of a direction holds
// positions 256w .. 256w+255, four consecutive ones a lane. Direction F runs
// alpha upward from frame 0, direction R beta downward from frame nf-1, they
// meet once at m = nf/2 and each emits the half of the frames it enters with
// its own vector in registers -- lt_align_post.hip's plan.
//
//   carry      Inside a wave position u-1 (F) / u+1 (R) is one lane shift
//              away. Across a wave boundary F's wave w needs, at frame t,
//              alpha_t[256w-1] + lex_t[256w-1]: lane 63's last term of wave
//              w-1 at the same frame; R's wave w needs beta_{t+1}[256(w+1)],
//              lane 0's first term of wave w+1. That pair is the fill value
//              of the receiving wave's shift (post_step's fo, fv).
//   pipeline   Frames are taken in blocks of kLongF. At block-step s the wave
//              of rank r (F: r = w, R: r = NW-1-w: the order the carries
//              travel in) runs block s-r of its direction, writes the block's
//              outgoing carries into an LDS ring [direction][NW-1][2][kLongF]
//              of float2 (double-buffered by block parity) and its neighbour
//              reads them one block-step later: ONE __syncthreads() per
//              block-step, none per frame. The step count is the same in all
//              2 NW waves (computed from nf alone); a wave with no block at a
//              step only passes the barrier.
//   phase 1    F stores alpha_t for t < m, R stores beta_{t+1} for t >= m into
//              the history [T, 256 NW] of (integer part, fraction) in the
//              caller's workspace (an aligned utterance has T >= U > 255:
//              the history never fits LDS). The pipeline drains.
//   midpoint   Every wave publishes its slice of alpha_m / beta_m in LDS, one
//              barrier, then every wave reduces all 256 NW positions from the
//              same LDS words by the same instructions: one log_prob,
//              bit-equal in all waves; the unaligned exit is workgroup-uniform.
//   phase 2    The pipeline refills. Each wave reads the other direction's
//              history row at columns u+1 (F) / u (R) -- from the workspace,
//              so that shift needs no carry -- and stores its 256 columns of
//              the frame's emission row.
// Weights and history rows run kD frames ahead through register rings across
// the blocks; a block's incoming carries are read once, one per lane, and
// handed out by v_readlane: no load sits on the chain. No atomics.
#include "lt_string_common.h"

namespace {

constexpr int kLongF = 16;  // frames of a pipeline block (tests/test_gpu_align_post_long.py: F)

struct PlArgs {
  const unsigned char* W;
  const int* nfr;
  const int* table;    // [C, V] next state of (p, y)
  const int* labels;   // [B, U]
  const int* nlab;     // [B]
  float* em;           // [B, T, U]
  float* lp;           // [B]
  float2* ws;          // history [B, T, 256 NW] (integer part, fraction)
  int B, T, U, C, V, R;
  int stage_tab;       // the next-state table is staged in LDS for the walk
};

LT_DEVINL float lane_value(float x, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l));
}

// One frame of the two recursions for a lane's P consecutive positions from
// u0 -- the frame step of lt_align_post.hip's post_phase, term for term, with
// the lane's first position and the shift's fill values as arguments. (It is
// written out here: post_phase calling it compiled to other machine code for
// align_post_kernel -- compare operands swapped, the selects after lae_split
// in another order -- and that kernel's code is pinned by its rerun and
// parity tests.)
// (o, v) is alpha_t (!REV) or beta_{t+1} (REV) as (integer part, fraction), wb
// / wl the frame's blank / lexical weights, and the step leaves alpha_{t+1} /
// beta_t in (o, v). PH2: hh is the other direction's history at the frame
// (beta_{t+1}[u+1] for !REV, alpha_t[u] for REV) and the frame's emission row
// er gets its columns u < U. (fo, fv) is what the wave shift hands the lane
// with no neighbour: alpha_t[u0-1] + lex_t[u0-1] in lane 0 (!REV) or
// beta_{t+1}[u0+P] in lane 63 (REV) -- (-inf, 0) where the string ends there,
// the neighbouring wave's carry where it goes on.
template <int P, bool REV, bool PH2>
LT_DEVINL void post_step(float (&o)[P], float (&v)[P], const float (&wb)[P], const float (&wl)[P],
                         const float2 (&hh)[P], float* er, int U, int u0, float fo, float fv,
                         float lpi, float lpf) {
  float no[P], nv[P];
  if constexpr (!REV) {
    // the arc leaving u: (o[j], lv[j]) = alpha_t[u] + lex_t[u]
    float lv[P];
#pragma unroll
    for (int j = 0; j < P; ++j) lv[j] = v[j] + wl[j];
    if constexpr (PH2) {
#pragma unroll
      for (int j = 0; j < P; ++j) {
        const int u = u0 + j;
        const float arg = (o[j] + hh[j].x - lpi) + (lv[j] + hh[j].y - lpf);
        if (u < U) er[u] = lt_exp(arg);
      }
    }
    const float po = wave_prev(o[P - 1], fo), pv = wave_prev(lv[P - 1], fv);
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const int u = u0 + j;
      const float lo = j ? o[j ? j - 1 : 0] : po, lf = j ? lv[j ? j - 1 : 0] : pv;
      lae_split(o[j], v[j] + wb[j], lo, lf, no[j], nv[j]);
      if (u > U) {
        no[j] = -kInf;
        nv[j] = 0.f;
      }
    }
  } else {
    const float nxo = wave_next(o[0], fo), nxv = wave_next(v[0], fv);
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const int u = u0 + j;
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

// One phase of wave w of a direction: steps i0..i1-1 (step i is frame t = i
// (F) or nf-1-i (R)) in blocks of kLongF, block k at block-step k + rank, and
// `nsteps` barriers whatever the wave has to do. ring: the direction's
// [NW-1][2][kLongF] carries; edge e is written by rank e and read by rank e+1.
template <bool BF16, int NW, bool REV, bool PH2>
LT_DEVINL void long_phase(const unsigned char* wbase, long long frame_bytes, const int (&ob)[4],
                          const int (&ol)[4], float (&o)[4], float (&v)[4], float2* hist, float* em,
                          int U, int lane, int w, int i0, int i1, int nf, int nsteps, float2* ring,
                          float lpi, float lpf) {
  constexpr int P = 4, SPT = 256 * NW, F = kLongF;
  constexpr int D = 8;  // frames of weights / history in flight; F is a multiple
  static_assert(F % D == 0, "a block is whole rounds of the register ring");
  const int rank = REV ? NW - 1 - w : w;
  const int u0 = 256 * w + lane * P;
  const bool has_in = rank > 0, has_out = rank < NW - 1;
  const float2* rin = ring + (has_in ? rank - 1 : 0) * 2 * F;
  float2* rout = ring + (has_out ? rank : 0) * 2 * F;
  // F reads beta_{t+1}[u+1], R reads alpha_t[u] (column SPT-1 is never a live arc)
  int hx[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int u = u0 + j;
    hx[j] = REV ? u : (u + 1 < SPT ? u + 1 : SPT - 1);
  }
  float pb[D][P], pl[D][P];
  float2 ph[D][P];
  if (i0 < i1) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int i = i0 + d < i1 ? i0 + d : i1 - 1;
      const int t = REV ? nf - 1 - i : i;
      const unsigned char* wf = wbase + (long long)t * frame_bytes;
#pragma unroll
      for (int j = 0; j < P; ++j) {
        pb[d][j] = ldw<BF16>(wf, ob[j]);
        pl[d][j] = ldw<BF16>(wf, ol[j]);
        if constexpr (PH2) ph[d][j] = hist[(long long)t * SPT + hx[j]];
      }
    }
  }
  for (int s = 0; s < nsteps; ++s) {
    const int k = s - rank;
    const int ib = i0 + k * F;
    if (k >= 0 && ib < i1) {
      // the block's incoming carries, frame f in lane f
      float2 cin = make_float2(-kInf, 0.f);
      if (has_in && lane < F) cin = rin[(k & 1) * F + lane];
      float2* co = rout + (k & 1) * F;
      for (int h = 0; h < F; h += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
          const int f = h + d, i = ib + f;
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
              if constexpr (PH2) ph[d][j] = hist[(long long)tn * SPT + hx[j]];
            }
          }
          if constexpr (!PH2) {
            float2* hr = hist + (long long)t * SPT + u0;
#pragma unroll
            for (int j = 0; j < P; ++j) hr[j] = make_float2(o[j], v[j]);
          }
          // what the next wave's shift takes in at this frame
          if (has_out && lane == (REV ? 0 : 63))
            co[f] = REV ? make_float2(o[0], v[0]) : make_float2(o[P - 1], v[P - 1] + wl[P - 1]);
          const float fo = lane_value(cin.x, f), fv = lane_value(cin.y, f);
          post_step<P, REV, PH2>(o, v, wb, wl, hh, em + (long long)t * U, U, u0, fo, fv, lpi, lpf);
        }
      }
    }
    __syncthreads();  // the block's carries
  }
}

// The one meeting of the 2 NW waves: each publishes its 256 positions of
// alpha_m (F) or beta_m (R) in mid [2, 256 NW], ONE barrier, then every wave
// computes log_prob = lpi + lpf = logsumexp_u(alpha_m[u] + beta_m[u]) over all
// positions (lane l: the four from 256k + 4l of every slice k) from the same
// LDS words by the same instructions: bit-equal in all waves. Returns whether
// any path carries weight (the same in all waves); lpi = 0 when none does.
template <int NW>
LT_DEVINL bool long_midpoint(float2* mid, bool rev, int w, int lane, const float (&o)[4],
                             const float (&v)[4], float& lpi, float& lpf) {
  constexpr int SPT = 256 * NW, N = 4 * NW;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    mid[(rev ? SPT : 0) + 256 * w + lane * 4 + j] = make_float2(o[j], v[j]);
  __syncthreads();  // history rows and the midpoint vectors
  float si[N], sf[N];
  float mx = -kInf;
#pragma unroll
  for (int n = 0; n < N; ++n) {
    const int u = 256 * (n / 4) + lane * 4 + n % 4;
    const float2 x = mid[u], y = mid[SPT + u];
    si[n] = x.x + y.x;
    sf[n] = x.y + y.y;
    mx = fmaxf(mx, si[n] + sf[n]);
  }
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) mx = fmaxf(mx, __shfl_xor(mx, s, 64));
  const bool ok = __builtin_isfinite(mx);
  lpi = ok ? floorf(mx) : 0.f;
  float sum = 0.f;
#pragma unroll
  for (int n = 0; n < N; ++n) sum += lt_exp((si[n] - lpi) + sf[n]);
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) sum += __shfl_xor(sum, s, 64);
  lpf = lt_log_acc(sum);
  return ok;
}

template <bool BF16, int NW>
__global__ __launch_bounds__(128 * NW) void align_post_long_kernel(const PlArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pl_sm[];
  constexpr int P = 4, SPT = 256 * NW, NT = 128 * NW, F = kLongF;
  constexpr int ES = BF16 ? 2 : 4;
  const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.x;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool rev = wid >= NW;  // direction R
  const int w = rev ? wid - NW : wid;
  const int U = a.U, T = a.T;
  int nf = a.nfr[b];
  nf = nf < 0 ? 0 : (nf > T ? T : nf);
  float* em = a.em + (long long)b * T * U;

  // ---- rows of padding frames
  for (long long i = (long long)nf * U + tid; i < (long long)T * U; i += NT) em[i] = 0.f;

  // ---- string positions: context state and label class
  int ob[P], ol[P];
  const StringLds sl = string_prologue<P, NT, 16, SPT>(a, b, tid, lane, pl_sm, ob, ol, 256 * w);
  float2* mid = (float2*)sl.mid;  // [2, SPT] alpha_m, beta_m
  // the carry ring takes the staged table's place
  float2* ring = (float2*)sl.region + (rev ? (NW - 1) * 2 * F : 0);

  const long long FRB = (long long)a.C * a.R * ES;
  const unsigned char* wbase = a.W + (long long)b * T * FRB;
  float2* hist = a.ws + (long long)b * T * SPT;
  const int nlb = a.nlab[b];
  const int fin = (nlb >= 0 && nlb <= U) ? nlb : -1;
  float o[P], v[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int u = 256 * w + lane * P + j;
    o[j] = (rev ? u == fin : u == 0) ? 0.f : -kInf;
    v[j] = 0.f;
  }
  const int m = nf / 2;
  const int n1 = rev ? nf - m : m;  // steps before the midpoint
  // block-steps of a phase: the longer half's blocks (nf - m >= m) and the skew
  const int nb = (nf - m + F - 1) / F;
  const int nsteps = nb ? nb + NW - 1 : 0;

  // ---- phase 1
  if (!rev)
    long_phase<BF16, NW, false, false>(wbase, FRB, ob, ol, o, v, hist, em, U, lane, w, 0, n1, nf,
                                       nsteps, ring, 0.f, 0.f);
  else
    long_phase<BF16, NW, true, false>(wbase, FRB, ob, ol, o, v, hist, em, U, lane, w, 0, n1, nf,
                                      nsteps, ring, 0.f, 0.f);

  // ---- the one meeting of all waves: log_prob, the same in each
  float lpi, lpf;
  const bool ok = long_midpoint<NW>(mid, rev, w, lane, o, v, lpi, lpf);
  if (tid == 0) a.lp[b] = ok ? lpi + lpf : -kInf;
  if (!ok) {  // unaligned: no path carries weight
    for (long long i = tid; i < (long long)nf * U; i += NT) em[i] = 0.f;
    return;
  }

  // ---- phase 2
  if (!rev)
    long_phase<BF16, NW, false, true>(wbase, FRB, ob, ol, o, v, hist, em, U, lane, w, n1, nf, nf,
                                      nsteps, ring, lpi, lpf);
  else
    long_phase<BF16, NW, true, true>(wbase, FRB, ob, ol, o, v, hist, em, U, lane, w, n1, nf, nf,
                                     nsteps, ring, lpi, lpf);
}

struct LongPlan {
  int NW, stage_tab, lds;
  size_t ws;
};

// Validates the shape and lays out LDS / workspace.
int long_plan(const lt_graph* g, const lt_table_problem* pb, LongPlan* pl) {
  if (int rc = table_check("lt_table_align_posteriors_long", g, pb, kChkString, [&] {
        if (g->expansions > 0)
          return fail(LT_EUNSUPPORTED,
                      "lt_table_align_posteriors_long: FrameLabelDependent (expansions >= 1)");
        if (pb->max_labels < 256 || pb->max_labels > 1023)
          return fail(LT_EUNSUPPORTED,
                      "lt_table_align_posteriors_long: max_labels outside 256..1023");
        return LT_OK;
      }))
    return rc;
  pl->NW = (pb->max_labels + 256) / 256;
  const long long SPT = 256LL * pl->NW;
  const long long stage = stage_table(g);
  pl->stage_tab = stage ? 1 : 0;
  // ctx, yn, yt; alpha_m, beta_m; then the staged table, and in its place the carry ring
  const long long ringb = 2LL * (pl->NW - 1) * 2 * kLongF * 8;
  const long long lds = (3 * 4 + 2 * 8) * SPT + ((std::max(stage, ringb) + 15) & ~15LL);
  if (lds > kTabLds)
    return fail(LT_EUNSUPPORTED, "lt_table_align_posteriors_long: the LDS layout does not fit");
  pl->lds = (int)lds;
  // a frame of history is (integer part, fraction) a position
  pl->ws = (size_t)(((long long)pb->batch * pb->max_frames * SPT * 8 + 255) & ~255LL);
  return LT_OK;
}

}  // namespace

extern "C" {

int lt_table_align_posteriors_long_workspace_bytes(const lt_graph* g, const lt_table_problem* pb,
                                                   size_t* bytes) {
  LongPlan pl;
  if (int rc = long_plan(g, pb, &pl)) return rc;
  if (bytes) *bytes = pl.ws;
  return LT_OK;
}

int lt_table_align_posteriors_long(const lt_graph* g, const lt_table_problem* pb, const void* W,
                                   const int32_t* num_frames, const int32_t* labels,
                                   const int32_t* num_labels, float* emission, float* log_prob,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  LongPlan pl;
  if (int rc = long_plan(g, pb, &pl)) return rc;
  if (pb->batch == 0) return LT_OK;
  if ((!W && pb->max_frames > 0) || !num_frames || !num_labels || !log_prob ||
      (!emission && pb->max_frames > 0) || !labels)
    return fail(LT_EINVAL, "null pointer");
  const bool bf16 = pb->weight_dtype == LT_DTYPE_BF16;
  if (((uintptr_t)W & (bf16 ? 1 : 3)) || ((uintptr_t)num_frames & 3) || ((uintptr_t)labels & 3) ||
      ((uintptr_t)num_labels & 3) || ((uintptr_t)emission & 3) || ((uintptr_t)log_prob & 3) ||
      ((uintptr_t)workspace & 7))
    return fail(LT_EINVAL, "misaligned pointer");
  if (pl.ws && (!workspace || workspace_bytes < pl.ws))
    return fail(LT_EINVAL, "workspace too small");
  PlArgs a;
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
  return dispatch(bf16, [&](auto bf) {
    constexpr bool BF16 = decltype(bf)::value;
    auto k = pl.NW == 2   ? align_post_long_kernel<BF16, 2>
             : pl.NW == 3 ? align_post_long_kernel<BF16, 3>
                          : align_post_long_kernel<BF16, 4>;
    return launch(k, dim3(a.B), dim3(128 * pl.NW), pl.lds, st, a, "long alignment posteriors");
  });
}

}  // extern "C"
