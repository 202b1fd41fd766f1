// lt_expect.hip -- posterior means of arc values on the denominator lattice
// (any next-state table x FrameDependent): E = sum_a m_a v_a, the arc
// marginals m_a = dE/dv_a and the covariances dE/dw_a = m_a (E[v | a] - E).
// The definition is in include/lt_expect.h.
//
// Two kernels, one workgroup per utterance, on the frame-serial skeleton of
// tab_fwd_k0_body / tab_bwd_den_k0_body (lt_table.hip, helpers shared through
// lt_table_common.h; the host checks and the launch through
// lt_string_common.h): one barrier a frame, the vectors double-buffered in LDS
// with Log's integer shift pending, the frame's W and values staged a frame
// ahead while they fit, the graph's CSR / table in LDS.
//   pair      every Log vector x (alpha, beta) travels with a linear-space
//             vector xm of conditional means (the mean prefix / suffix value
//             given the state). A reduction over arcs keeps (max, sum e^{x-max},
//             sum e^{x-max} (xm + v)), rescaled when the max moves: one pass
//             gives the new x = max + log sum and xm = third / second. No log
//             of a value sum, so values may have any sign.
//   select    an arc of weight -inf adds nothing, and its value is never
//             multiplied (a NaN there is harmless).
//   forward   G = 8 lanes a state over its in-arcs (the blank arc is candidate
//             0), writes alpha_t and its means to the workspace, then log_z, E.
//   backward  frames nf-1 .. 0, G lanes a source state over its V+1 out-arcs:
//             the same pass emits marg and cov (a group's lanes store
//             consecutive elements of the row) and reduces beta and its means.
// No atomics on memory; the only LDS atomic is the shift slot's integer max,
// which is order-independent, so two calls give bit-equal outputs.
#include "lt_string_common.h"

namespace {

struct EArgs {
  const unsigned char* W;
  const float* val;   // [B,T,C,V+1]
  const int* nfr;
  const int* table;   // [C, V] next state of (p, y)
  const int* in_off;  // [C+1]
  const int* in_arc;  // [C*V] arc id p*V + (y-1), grouped by next state
  float* expected;    // [B]
  float* logz;        // [B]
  float* ha;          // workspace: alpha history [B,T,C] (null: not kept)
  float* hm;          // workspace: its means [B,T,C]
  float* marg;        // [B,T,C,V+1], nullable
  float* cov;         // [B,T,C,V+1], nullable
  int B, T, C, V, R;
};

constexpr int kExpG = 8;  // lanes per state

// The running triple of a softmax-weighted mean: log-sum m + log s, mean u / s.
struct MeanAcc {
  float m = -kInf, s = 0.f, u = 0.f;
  // folds N terms (x[i], e[i]); a term with x = -inf is skipped and its e is
  // not read into the arithmetic
  template <int N>
  LT_DEVINL void fold(const float (&x)[N], const float (&e)[N]) {
    float cm = x[0];
#pragma unroll
    for (int i = 1; i < N; ++i) cm = fmaxf(cm, x[i]);
    if (cm == kInf) {  // +inf dominates: log_z is not finite, the mean is unused
      m = kInf;
      s = 1.f;
      u = 0.f;
    } else if (cm != -kInf && m != kInf) {
      float cs = 0.f, cu = 0.f;
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const float w = lt_exp(x[i] - cm);
        cs += w;
        cu += x[i] > -kInf ? w * e[i] : 0.f;
      }
      const float M = fmaxf(m, cm);
      const float ca = lt_exp(m - M), cb = lt_exp(cm - M);
      s = s * ca + cs * cb;
      u = u * ca + cu * cb;
      m = M;
    }
  }
  // merges the triples of G aligned lanes (xor shuffles; every lane of the
  // wave takes part): the lanes then hold the group's total
  template <int G>
  LT_DEVINL void merge() {
    for (int o = 1; o < G; o <<= 1) {
      const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
      const float u2 = __shfl_xor(u, o, 64);
      const float M = fmaxf(m, m2);
      if (M == -kInf) {
        s = 0.f;
        u = 0.f;
      } else {
        const float ca = m == M ? 1.f : lt_exp(m - M), cb = m2 == M ? 1.f : lt_exp(m2 - M);
        s = s * ca + s2 * cb;
        u = u * ca + u2 * cb;
        m = M;
      }
    }
  }
  LT_DEVINL float log() const { return s > 0.f ? m + lt_log_acc(s) : -kInf; }
  LT_DEVINL float mean() const { return s > 0.f ? u / s : 0.f; }
};

// LDS layout (floats) after the graph copy: fwd 4C, bwd 8C, then when staged
// W [2][FR] and values [2][FR]
LT_DEVINL float* e_base(const EArgs& a, float* sm, bool stage) {
  return sm + (stage ? (a.C + 1 + 2 * a.C * a.V + 3) / 4 * 4 : 0);
}

// ---- forward: alpha_t with its means, log_z and E ---------------------------
template <bool BF16, bool STAGE>
LT_DEVINL void expect_fwd_body(const EArgs& a, const int b, float* sm) {
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int S = a.C, R = a.R;
  const int* g_off;
  const int* g_arc;
  const int* g_tab;
  t_graph<STAGE>(a, (int*)sm, &g_off, &g_arc, &g_tab);
  (void)g_tab;
  float* base = e_base(a, sm, STAGE);
  float* cur = base;           // [S] alpha_t (unshifted)
  float* nxt = base + S;       // [S]
  float* mcur = base + 2 * S;  // [S] its means
  float* mnxt = base + 3 * S;  // [S]
  const long long FR = (long long)a.C * R;
  float* w0 = base + 4 * S;  // STAGE: [2][FR]
  float* v0 = w0 + 2 * FR;   // STAGE: [2][FR]
  int nf = a.nfr[b];
  nf = nf < 0 ? 0 : (nf > a.T ? a.T : nf);
  for (int q = tid; q < S; q += nthr) {
    cur[q] = q == 0 ? 0.f : -kInf;
    mcur[q] = 0.f;
  }
  __shared__ int slot_mem[3];
  const MaxSlots slots{slot_mem};
  slots.init();
  using DG = typename std::conditional<STAGE, DenGraphP, DenGraph>::type;
  const DG dg{g_off, g_arc, a.V, R};
  constexpr int G = kExpG, NU = 8;
  const long long fbytes = FR * (BF16 ? 2 : 4);
  const unsigned char* wb = a.W + (long long)b * a.T * fbytes;
  const unsigned char* vb = (const unsigned char*)(a.val + (long long)b * a.T * FR);
  FrameStage<BF16> fw;
  FrameStage<false> fv;
  if (STAGE && nf > 0) {
    fw.fetch(wb, FR);
    fv.fetch(vb, FR);
    fw.store(w0, wb, FR);
    fv.store(v0, vb, FR);
    fw.fetch(nf > 1 ? wb + fbytes : nullptr, FR);
    fv.fetch(nf > 1 ? vb + 4 * FR : nullptr, FR);
  }
  __syncthreads();
  float O = 0.f, sp = 0.f;  // the offset of cur - sp (sp included)
  const int jg = tid & (G - 1);
  for (int t = 0; t < nf; ++t) {
    if (t >= 1) {  // frame t - 1's shift, once
      sp = slots.shift(t - 1);
      O += sp;
    }
    if (a.ha)
      for (int q = tid; q < S; q += nthr) {
        a.ha[((long long)b * a.T + t) * S + q] = O + (cur[q] - sp);
        a.hm[((long long)b * a.T + t) * S + q] = mcur[q];
      }
    const unsigned char* wf = wb + t * fbytes;
    const float* vf = (const float*)(vb + t * 4 * FR);
    const float* wl = w0 + (t & 1) * FR;
    const float* vl = v0 + (t & 1) * FR;
    auto wr = [&](int i) { return STAGE ? wl[i] : ldw<BF16>(wf, i); };
    auto vr = [&](int i) { return STAGE ? vl[i] : vf[i]; };
    for (int q0 = 0; q0 < S; q0 += nthr / G) {
      const int q = q0 + tid / G;
      const bool valid = q < S;
      // candidates of q: 0 the blank self-arc, k >= 1 in-arc k - 1 of the CSR
      const int n = valid ? dg.nin(q) + 1 : 0, p0 = valid ? dg.pos0(q) : 0;
      MeanAcc acc;
      for (int k0 = jg; k0 < n; k0 += G * NU) {
        float x[NU], e[NU];
#pragma unroll
        for (int i = 0; i < NU; ++i) {
          const int k = k0 + G * i;
          x[i] = -kInf;
          e[i] = 0.f;
          if (k < n) {
            int src = q, wi = dg.blank(q);
            if (k > 0) dg.arc(p0 + k - 1, q, &src, &wi);
            x[i] = (cur[src] - sp) + wr(wi);
            e[i] = mcur[src] + vr(wi);
          }
        }
        acc.fold<NU>(x, e);
      }
      acc.merge<G>();
      if (!valid || jg) continue;
      const float o = acc.log();
      nxt[q] = o;
      mnxt[q] = acc.mean();
      slots.put(t, o);
    }
    if (STAGE && t + 1 < nf) {  // frame t + 1 into the other buffers, t + 2 in flight
      fw.store(w0 + ((t + 1) & 1) * FR, wf + fbytes, FR);
      fv.store(v0 + ((t + 1) & 1) * FR, (const unsigned char*)(vf + FR), FR);
      fw.fetch(t + 2 < nf ? wf + 2 * fbytes : nullptr, FR);
      fv.fetch(t + 2 < nf ? (const unsigned char*)(vf + 2 * FR) : nullptr, FR);
    }
    slots.reset_next(t);
    __syncthreads();
    float* tmp = cur;
    cur = nxt;
    nxt = tmp;
    tmp = mcur;
    mcur = mnxt;
    mnxt = tmp;
  }
  if (nf >= 1) {  // the last frame's shift
    sp = slots.shift(nf - 1);
    O += sp;
  }
  if (tid < 64) {  // log_z = (+)_q alpha_T[q] and E = the posterior mean of the means
    MeanAcc acc;
    for (int q = tid; q < S; q += 64) {
      const float x[1] = {cur[q] - sp}, e[1] = {mcur[q]};
      acc.fold<1>(x, e);
    }
    acc.merge<64>();
    if (tid == 0) {
      const float lz = O + acc.log();
      a.logz[b] = lz;
      a.expected[b] = __builtin_isfinite(lz) ? acc.mean() : 0.f;
    }
  }
}

// ---- backward: beta with its means, marg and cov ----------------------------
template <bool BF16, bool STAGE>
LT_DEVINL void expect_bwd_body(const EArgs& a, const int b, float* sm) {
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int C = a.C, V = a.V, R = a.R;
  const int* g_off;
  const int* g_arc;
  const int* g_tab;
  t_graph<STAGE>(a, (int*)sm, &g_off, &g_arc, &g_tab);
  (void)g_off;
  (void)g_arc;
  float* base = e_base(a, sm, STAGE);
  float* cur = base;           // [C] beta_{t+1} (unshifted)
  float* nxt = base + C;       // [C]
  float* mcur = base + 2 * C;  // [C] its means
  float* mnxt = base + 3 * C;  // [C]
  float* la0 = base + 4 * C;   // [2][C] alpha rows
  float* lm0 = base + 6 * C;   // [2][C] rows of alpha's means
  const long long FR = (long long)C * R;
  float* w0 = base + 8 * C;  // STAGE: [2][FR]
  float* v0 = w0 + 2 * FR;   // STAGE: [2][FR]
  int nf = a.nfr[b];
  nf = nf < 0 ? 0 : (nf > a.T ? a.T : nf);
  const float lz = a.logz[b];
  const float E = a.expected[b];
  if (!__builtin_isfinite(lz)) nf = 0;  // workgroup-uniform: zero gradients
  // padding frames (every frame of an utterance without a finite log_z)
  {
    const long long z0 = ((long long)b * a.T + nf) * FR, zn = (long long)(a.T - nf) * FR;
    for (long long e = tid; e < zn; e += nthr) {
      if (a.marg) a.marg[z0 + e] = 0.f;
      if (a.cov) a.cov[z0 + e] = 0.f;
    }
  }
  if (nf == 0) return;
  for (int q = tid; q < C; q += nthr) {  // every state final
    cur[q] = 0.f;
    mcur[q] = 0.f;
  }
  __shared__ int slot_mem[3];
  const MaxSlots slots{slot_mem};
  slots.init();
  constexpr int G = kExpG, NU = 4;
  const int esz = BF16 ? 2 : 4;
  auto lda = [&](int t) {  // rows of frame t, gathered one frame ahead
    return [=](int e) { return a.ha[((long long)b * a.T + t) * C + e]; };
  };
  auto ldm = [&](int t) {
    return [=](int e) { return a.hm[((long long)b * a.T + t) * C + e]; };
  };
  FrameStage<BF16> fw;
  FrameStage<false> fv;
  RegStage<1> hsa, hsm;
  {
    const unsigned char* wl = a.W + ((long long)b * a.T + nf - 1) * FR * esz;
    const unsigned char* vl = (const unsigned char*)(a.val + ((long long)b * a.T + nf - 1) * FR);
    if (STAGE) {
      fw.fetch(wl, FR);
      fv.fetch(vl, FR);
      fw.store(w0 + ((nf - 1) & 1) * FR, wl, FR);
      fv.store(v0 + ((nf - 1) & 1) * FR, vl, FR);
      fw.fetch(nf > 1 ? wl - FR * esz : nullptr, FR);
      fv.fetch(nf > 1 ? vl - FR * 4 : nullptr, FR);
    }
    hsa.fetch(C, lda(nf - 1));
    hsm.fetch(C, ldm(nf - 1));
    hsa.store(la0 + ((nf - 1) & 1) * C, C, lda(nf - 1));
    hsm.store(lm0 + ((nf - 1) & 1) * C, C, ldm(nf - 1));
    hsa.fetch(nf > 1 ? C : 0, lda(nf - 2));
    hsm.fetch(nf > 1 ? C : 0, ldm(nf - 2));
  }
  __syncthreads();
  float Ob = 0.f, sp = 0.f;
  const int jg = tid & (G - 1);
  for (int t = nf - 1; t >= 0; --t) {
    const int it = nf - 1 - t;  // the order the frames run in (the slots rotate with it)
    const long long fo = ((long long)b * a.T + t) * FR;
    if (it >= 1) {  // frame t + 1's shift, once
      sp = slots.shift(it - 1);
      Ob += sp;
    }
    const unsigned char* wf = a.W + fo * esz;
    const float* vf = a.val + fo;
    const float* wl = w0 + (t & 1) * FR;
    const float* vl = v0 + (t & 1) * FR;
    const float* la = la0 + (t & 1) * C;
    const float* lm = lm0 + (t & 1) * C;
    auto wr = [&](int i) { return STAGE ? wl[i] : ldw<BF16>(wf, i); };
    auto vr = [&](int i) { return STAGE ? vl[i] : vf[i]; };
    // G lanes per source state p: lane jg takes the out-arcs y = jg, jg + G, ...
    // (y = 0 the blank arc, which stays in p)
    for (int p0 = 0; p0 < C; p0 += nthr / G) {
      const int p = p0 + tid / G;
      const bool valid = p < C;
      const float a0 = valid ? (la[p] - lz) + Ob : -kInf;  // log of the prefix posterior mass
      const float am = valid ? lm[p] - E : 0.f;
      const bool reach = a0 > -kInf;
      MeanAcc acc;
      for (int y0 = jg; valid && y0 <= V; y0 += G * NU) {
        float x[NU], e[NU];
#pragma unroll
        for (int i = 0; i < NU; ++i) {
          const int y = y0 + G * i;
          x[i] = -kInf;
          e[i] = 0.f;
          if (y <= V) {
            const int q = y == 0 ? p : g_tab[p * V + y - 1];
            x[i] = wr(p * R + y) + (cur[q] - sp);
            e[i] = vr(p * R + y) + mcur[q];
            const bool on = reach && x[i] > -kInf;
            const float mg = on ? lt_exp(a0 + x[i]) : 0.f;
            if (a.marg) a.marg[fo + p * R + y] = mg;
            if (a.cov) a.cov[fo + p * R + y] = on ? mg * (am + e[i]) : 0.f;
          }
        }
        acc.fold<NU>(x, e);
      }
      acc.merge<G>();
      if (!valid || jg) continue;
      const float o = acc.log();
      nxt[p] = o;
      mnxt[p] = acc.mean();
      slots.put(it, o);
    }
    if (t >= 1) {  // frame t - 1's weights, values and history rows into the other buffers
      if (STAGE) {
        fw.store(w0 + ((t - 1) & 1) * FR, wf - FR * esz, FR);
        fv.store(v0 + ((t - 1) & 1) * FR, (const unsigned char*)(vf - FR), FR);
        fw.fetch(t >= 2 ? wf - 2 * FR * esz : nullptr, FR);
        fv.fetch(t >= 2 ? (const unsigned char*)(vf - 2 * FR) : nullptr, FR);
      }
      hsa.store(la0 + ((t - 1) & 1) * C, C, lda(t - 1));
      hsm.store(lm0 + ((t - 1) & 1) * C, C, ldm(t - 1));
      hsa.fetch(t >= 2 ? C : 0, lda(t - 2));
      hsm.fetch(t >= 2 ? C : 0, ldm(t - 2));
    }
    slots.reset_next(it);
    __syncthreads();
    float* tmp = cur;
    cur = nxt;
    nxt = tmp;
    tmp = mcur;
    mcur = mnxt;
    mnxt = tmp;
  }
}

template <bool BF16, bool STAGE>
__global__ __launch_bounds__(512) void expect_fwd_kernel(const EArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  expect_fwd_body<BF16, STAGE>(a, (int)blockIdx.x, sm);
}

template <bool BF16, bool STAGE>
__global__ __launch_bounds__(512) void expect_bwd_kernel(const EArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  expect_bwd_body<BF16, STAGE>(a, (int)blockIdx.x, sm);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct ExpectPlan {
  int stage;             // graph and frames in LDS
  int lds_fwd, lds_bwd;  // dynamic LDS bytes
  int threads;
  size_t hm, total;  // workspace: alpha history at 0, its means at hm
};

// Validates the shape and lays out LDS and the workspace.
int expect_plan(const lt_graph* g, const lt_table_problem* pb, ExpectPlan* pl) {
  if (int rc = table_check("lt_table_expectation", g, pb, 0, [&] {
        if (g->expansions >= 1)
          return fail(LT_EUNSUPPORTED,
                      "lt_table_expectation: FrameLabelDependent is not supported");
        return check_arrays(g, true);
      }))
    return rc;
  const long long C = g->num_states, V = g->vocab_size, FR = C * (V + 1);
  // the table kernels' LDS rule: frames and graph staged while the larger
  // (backward) image fits the staging budget, else only the vectors in LDS
  const long long vec_f = 4 * 4 * C, vec_b = 4 * 8 * C;
  const long long graph = 4 * ((C + 1 + 2 * C * V + 3) / 4 * 4);
  pl->stage = vec_b + graph + 16 * FR <= kStageBudget;
  const long long lf = pl->stage ? vec_f + graph + 16 * FR : vec_f;
  const long long lb = pl->stage ? vec_b + graph + 16 * FR : vec_b;
  if (lb > kTabLds) return fail(LT_EUNSUPPORTED, "table lattice state exceeds LDS");
  pl->lds_fwd = (int)lf;
  pl->lds_bwd = (int)lb;
  // 8 lanes per state: 512 threads cover up to 64 states in one pass
  pl->threads = C > 32 ? 512 : 256;
  const long long hist = 4LL * pb->batch * pb->max_frames * C;
  pl->hm = (size_t)((hist + 255) & ~255LL);
  pl->total = 2 * pl->hm;
  return LT_OK;
}

template <bool BF16>
int expect_run(const EArgs& a, const ExpectPlan& pl, bool bwd, hipStream_t st) {
  const dim3 grid((unsigned)a.B), block(pl.threads);
  auto fwd = pl.stage ? expect_fwd_kernel<BF16, true> : expect_fwd_kernel<BF16, false>;
  const int rc = launch(fwd, grid, block, pl.lds_fwd, st, a, "expectation", " forward launch");
  if (rc || !bwd) return rc;
  auto bk = pl.stage ? expect_bwd_kernel<BF16, true> : expect_bwd_kernel<BF16, false>;
  return launch(bk, grid, block, pl.lds_bwd, st, a, "expectation", " backward launch");
}

}  // namespace

extern "C" {

int lt_table_expectation_workspace_bytes(const lt_graph* g, const lt_table_problem* pb,
                                         size_t* bytes) {
  ExpectPlan pl;
  if (int rc = expect_plan(g, pb, &pl)) return rc;
  if (bytes) *bytes = pl.total;
  return LT_OK;
}

int lt_table_expectation(const lt_graph* g, const lt_table_problem* pb, const void* W,
                         const float* values, const int32_t* num_frames, float* expected,
                         float* log_z, float* marg, float* cov, void* workspace,
                         size_t workspace_bytes, void* stream) {
  ExpectPlan pl;
  if (int rc = expect_plan(g, pb, &pl)) return rc;
  if (!expected || !log_z) return fail(LT_EINVAL, "lt_table_expectation: null output");
  if (pb->batch == 0) return LT_OK;
  if (!num_frames || ((!W || !values) && pb->max_frames > 0))
    return fail(LT_EINVAL, "null pointer");
  if (pl.total && (!workspace || workspace_bytes < pl.total))
    return fail(LT_EINVAL, "workspace too small");
  if (((uintptr_t)workspace & 3) || ((uintptr_t)values & 3) || ((uintptr_t)marg & 3) ||
      ((uintptr_t)cov & 3) || ((uintptr_t)W & (pb->weight_dtype == LT_DTYPE_BF16 ? 1 : 3)))
    return fail(LT_EINVAL, "misaligned pointer");
  const bool bwd = (marg || cov) && pb->max_frames > 0;
  EArgs a;
  memset(&a, 0, sizeof(a));
  a.W = (const unsigned char*)W;
  a.val = values;
  a.nfr = num_frames;
  a.table = g->next_state;
  a.in_off = g->in_offsets;
  a.in_arc = g->in_arcs;
  a.expected = expected;
  a.logz = log_z;
  a.ha = bwd ? (float*)workspace : nullptr;  // a value-only call keeps no history
  a.hm = bwd ? (float*)((char*)workspace + pl.hm) : nullptr;
  a.marg = marg;
  a.cov = cov;
  a.B = pb->batch;
  a.T = pb->max_frames;
  a.C = g->num_states;
  a.V = g->vocab_size;
  a.R = g->vocab_size + 1;
  hipStream_t st = (hipStream_t)stream;
  return dispatch(pb->weight_dtype == LT_DTYPE_BF16, [&](auto bf) {
    return expect_run<decltype(bf)::value>(a, pl, bwd, st);
  });
}

}  // extern "C"
