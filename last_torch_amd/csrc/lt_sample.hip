// lt_sample.hip -- sampling alignment paths from the lattice posterior
// p(pi) = exp(w(pi)) / Z of the denominator lattice (any next-state table x
// FrameDependent): Gumbel-max over the arcs into the current state, walked
// backwards over the alpha history of lt_table_forward / lt_den_forward. The
// draw is specified in include/lt_sample.h (Philox4x32-10 keyed by the seed,
// counter (k >> 2, t, s, b)), so the paths do not depend on the launch.
//
// One wave per (utterance, sample); the waves of a workgroup belong to one
// utterance.
//   ring      the frames a walk visits are known in advance (nf-1 down to 0),
//             only the row inside a frame depends on the state. The workgroup
//             stages whole frames -- W [C, V+1] and alpha_t [C] -- one slice
//             of L frames ahead into a two-slice LDS ring: 16-byte loads
//             issued before a slice is walked, written to the other half
//             after it, one barrier a slice. Every sampling wave takes
//             exactly one step a frame, so the barrier orders the ring.
//   step      lane j scores candidate j of the state (the blank arc and the
//             in-arcs, from the CSR staged in LDS as (k, p) pairs while it
//             fits): an LDS gather, Philox, two v_log_f32, a six-stage DPP
//             max over the wave, one ballot of the lanes that hold it (equal
//             scores: the smallest k) and three v_readlane; more than 64
//             candidates go in slices of 64 with a running best. The last
//             live frame scans all arcs.
//   no ring   a frame larger than a slice (the V = 32 trigram: 139 KB) is
//             gathered from memory, one dependent access a step; no barrier.
//   labels    lane t % 64 keeps frame t's label; 64 frames go out as one
//             coalesced store, and the whole wave zero-fills the padding.
#include "lt_string_common.h"

namespace {

struct SArgs {
  const unsigned char* W;
  const int* nfr;
  const float* logz;
  const float* alpha;
  const int* table;    // [C, V] next state of (p, y)
  const int* in_off;   // [C+1]
  const int* in_arc;   // [C*V] arc ids p*V + y-1 grouped by next state
  long long* out;      // [B, S, T]
  float* pw;           // [B, S]
  unsigned key0, key1;
  int B, T, C, V, R, S;
  int wpb;        // sampling waves per workgroup
  int nblk;       // workgroups per utterance
  int L;          // frames per ring slice (0: no ring)
  int capW, capA; // 16-byte chunks of a slice's W / alpha image
  int stage_csr;  // the in-arc CSR is staged in LDS as (k, p) pairs
};

constexpr int kSampleKpt = 4;             // 16-byte loads a thread holds per slice
constexpr int kSampleCsr = 48 * 1024;     // largest image of the in-arc CSR staged in LDS
constexpr int kNoArc = 0x7fffffff;

// Philox4x32-10 (Random123): word k & 3 of the block (k >> 2, t, s, b).
LT_DEVINL unsigned philox_word(unsigned k, unsigned t, unsigned s, unsigned b, unsigned key0,
                               unsigned key1) {
  unsigned c0 = k >> 2, c1 = t, c2 = s, c3 = b;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    // both words of a product from one 32 x 32 -> 64 bit multiply
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    c0 = (unsigned)(p1 >> 32) ^ c1 ^ key0;
    c1 = (unsigned)p1;
    c2 = (unsigned)(p0 >> 32) ^ c3 ^ key1;
    c3 = (unsigned)p0;
    key0 += 0x9E3779B9u;
    key1 += 0xBB67AE85u;
  }
  const unsigned lo = (k & 1) ? c1 : c0, hi = (k & 1) ? c3 : c2;
  return (k & 2) ? hi : lo;
}

// -log(-log u), u = ((r >> 8) + 0.5) 2^-24, branch-free on v_log_f32 (whose
// error is about an ulp of log2 x). Below 1/2 u is an fp32 number. Above,
// fl(u) is off by d = u - fl(u) in {0, +-2^-25}, which is exact as
// (1 - fl(u)) - v with v = 1 - u exact: log u = log fl(u) + d / fl(u) to
// second order. Within 2^-6 of 1, where log2 fl(u) is a handful of ulps of
// 1 - fl(u), -log u is the series v + v^2/2 + v^3/3 + v^4/4 (truncation
// below 2^-26 of it).
LT_DEVINL float gumbel(unsigned r) {
  constexpr float kLn2 = 0.6931471805599453f;
  const unsigned x = r >> 8;
  const float u = ((float)x + 0.5f) * 0x1p-24f;
  const float v = (float)((1u << 25) - 2u * x - 1u) * 0x1p-25f;
  const float d = x < (1u << 23) ? 0.f : (1.f - u) - v;
  float e = -__builtin_fmaf(__builtin_amdgcn_logf(u), kLn2, d * __builtin_amdgcn_rcpf(u));
  const float es = v * (1.f + v * (0.5f + v * (0.33333334f + v * 0.25f)));
  e = v < 0x1p-6f ? es : e;
  return -kLn2 * __builtin_amdgcn_logf(e);
}

struct Pick {
  float v;  // best score
  int k;    // its arc, p*(V+1) + y
  int p;    // its source state
  float w;  // its weight
};

// Folds one slice of at most 64 candidates (lane: ok, arc k from state p, in
// the frame at wf / af) into the running best. Wave-uniform result. The whole
// wave must be active.
template <bool BF16>
LT_DEVINL void fold_slice(Pick& best, bool ok, int k, int p, const unsigned char* wf,
                          const float* af, unsigned t, unsigned s, unsigned b, const SArgs& a) {
  float sc = -kInf, w = 0.f;
  if (ok) {
    w = ldw<BF16>(wf, k);
    const float aw = af[p] + w;
    sc = aw + gumbel(philox_word((unsigned)k, t, s, b, a.key0, a.key1));
    if (!(sc == sc)) sc = -kInf;  // a NaN score never wins
  }
  const float top = wave_max(sc);
  unsigned long long m = __ballot(ok && sc == top);
  if (m == 0) return;  // no candidate in this slice
  int src = __ffsll((long long)m) - 1;
  int kw = __builtin_amdgcn_readlane(k, src);
  for (m &= m - 1; m; m &= m - 1) {  // equal scores (rare): the smallest k
    const int l = __ffsll((long long)m) - 1;
    const int kl = __builtin_amdgcn_readlane(k, l);
    if (kl < kw) {
      kw = kl;
      src = l;
    }
  }
  if (top > best.v || (top == best.v && kw < best.k)) {
    best.v = top;
    best.k = kw;
    best.p = __builtin_amdgcn_readlane(p, src);
    best.w = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), src));
  }
}

// The ring's slice i of an utterance: frames [tb - L, tb), tb = nf - i*L, as
// two byte ranges (W, alpha) widened to whole 16-byte granules.
struct SliceGeom {
  const unsigned char* w;  // the utterance's W
  const unsigned char* al; // the utterance's alpha
  long long fw, fa;        // bytes of a frame of each
  int nf, L, capW;
};
struct SliceRange {
  unsigned long long gw, ga;  // 16-byte aligned starts
  int nW, nA;                 // granules
};
LT_DEVINL SliceRange slice_range(const SliceGeom& g, int i) {
  const int tb = g.nf - i * g.L, ta = tb - g.L > 0 ? tb - g.L : 0;
  const unsigned long long gw = (unsigned long long)(g.w + (long long)ta * g.fw);
  const unsigned long long ga = (unsigned long long)(g.al + (long long)ta * g.fa);
  SliceRange r;
  r.nW = (int)(((gw & 15) + (unsigned long long)(tb - ta) * g.fw + 15) >> 4);
  r.nA = (int)(((ga & 15) + (unsigned long long)(tb - ta) * g.fa + 15) >> 4);
  r.gw = gw & ~15ull;
  r.ga = ga & ~15ull;
  return r;
}
// granule j of the slice (granules past it repeat its first one: always in
// range, never stored)
LT_DEVINL uint4 granule_load(const SliceRange& r, int j) {
  unsigned long long src = r.gw;
  if (j < r.nW) src = r.gw + 16ull * j;
  else if (j - r.nW < r.nA) src = r.ga + 16ull * (j - r.nW);
  return *(const uint4*)src;
}
LT_DEVINL void granule_store(const SliceRange& r, int j, unsigned char* buf, int capW,
                             const uint4& v) {
  if (j < r.nW) *(uint4*)(buf + 16 * j) = v;
  else if (j - r.nW < r.nA) *(uint4*)(buf + 16 * (capW + j - r.nW)) = v;
}
// thread tid holds granules tid + k*NT, k < kSampleKpt = 4, in four registers
// (named, so that they stay registers across the walk)
#define LT_SLICE_LOAD(i)                                      \
  {                                                           \
    const SliceRange r_ = slice_range(sg, (i));               \
    rg0 = granule_load(r_, tid);                              \
    rg1 = granule_load(r_, tid + NT);                         \
    rg2 = granule_load(r_, tid + 2 * NT);                     \
    rg3 = granule_load(r_, tid + 3 * NT);                     \
  }
#define LT_SLICE_STORE(i)                                     \
  {                                                           \
    const SliceRange r_ = slice_range(sg, (i));               \
    unsigned char* buf_ = s_sm + ((i) & 1) * sliceB;          \
    granule_store(r_, tid, buf_, sg.capW, rg0);               \
    granule_store(r_, tid + NT, buf_, sg.capW, rg1);          \
    granule_store(r_, tid + 2 * NT, buf_, sg.capW, rg2);      \
    granule_store(r_, tid + 3 * NT, buf_, sg.capW, rg3);      \
  }
static_assert(kSampleKpt == 4, "LT_SLICE_LOAD / LT_SLICE_STORE hold four granules");

template <bool BF16, bool RING>
__global__ __launch_bounds__(512) void sample_kernel(const SArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_sm[];
  constexpr int ES = BF16 ? 2 : 4;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int NT = blockDim.x;
  const int b = blockIdx.x / a.nblk;
  const int s = (blockIdx.x % a.nblk) * a.wpb + wave;
  const bool active = wave < a.wpb && s < a.S;
  const int T = a.T, C = a.C, R = a.R;
  int nf = a.nfr[b];
  nf = nf < 0 ? 0 : (nf > T ? T : nf);
  const float lz = a.logz[b];
  const bool sampled = __builtin_isfinite(lz);

  const int sliceB = RING ? 16 * (a.capW + a.capA) : 0;
  // the staged CSR: per state its candidates as (k, p) pairs, the blank arc
  // first, and seg[q] = (first pair, number of pairs)
  int2* seg = (int2*)(s_sm + 2 * sliceB);  // [C]
  int2* pair = seg + C;                    // [C*V + C]
  if (a.stage_csr) {
    for (int i = tid; i < C; i += NT) {
      const int o = a.in_off[i];
      seg[i] = make_int2(o + i, a.in_off[i + 1] - o + 1);
      pair[o + i] = make_int2(i * R, i);
    }
    for (int i = tid; i < C * a.V; i += NT) {
      const int id = a.in_arc[i];  // p*V + y-1: also its place in the table
      const int p = id / a.V;
      pair[i + a.table[id] + 1] = make_int2(p * R + (id - p * a.V) + 1, p);
    }
  }

  long long* out = active ? a.out + ((long long)b * a.S + s) * T : nullptr;
  if (active) {
    // padding frames past the last label chunk (all of the row when unsampled)
    const int from = (sampled && nf > 0) ? ((nf + 63) & ~63) : 0;
    for (int i = from + lane; i < T; i += 64) out[i] = 0;
  }
  if (!sampled || nf == 0) {  // workgroup-uniform
    if (active && lane == 0) a.pw[(long long)b * a.S + s] = sampled ? 0.f : -kInf;
    return;
  }

  const long long FWb = (long long)C * R * ES;  // bytes of a frame of W
  const unsigned char* wutt = a.W + (long long)b * T * FWb;
  const float* autt = a.alpha + (long long)b * T * C;

  // ---- ring staging: slice i covers frames [tb - L, tb), tb = nf - i*L
  uint4 rg0 = {}, rg1 = {}, rg2 = {}, rg3 = {};
  const SliceGeom sg = {wutt, (const unsigned char*)autt, FWb, (long long)C * 4, nf, a.L, a.capW};
  const int nsl = RING ? (nf + a.L - 1) / a.L : 1;
  if constexpr (RING) {
    LT_SLICE_LOAD(0)
    LT_SLICE_STORE(0)
  }
  if (RING || a.stage_csr) __syncthreads();

  int q = 0;
  float wsum = 0.f;
  long long lab = 0;  // lane t % 64: the label of frame t of the current chunk
  for (int i = 0; i < nsl; ++i) {
    const int tb = RING ? nf - i * a.L : nf;
    const int ta = RING ? (tb - a.L > 0 ? tb - a.L : 0) : 0;
    if constexpr (RING)
      if (i + 1 < nsl) LT_SLICE_LOAD(i + 1)
    if (active) {
      const unsigned char* wsl;
      const float* asl;
      if constexpr (RING) {
        const unsigned char* buf = s_sm + (i & 1) * sliceB;
        const unsigned long long gw = (unsigned long long)(wutt + (long long)ta * FWb);
        const unsigned long long ga = (unsigned long long)(autt + (long long)ta * C);
        wsl = buf + (gw & 15);
        asl = (const float*)(buf + 16 * a.capW + (ga & 15));
      } else {
        wsl = wutt;
        asl = autt;
      }
      for (int t = tb - 1; t >= ta; --t) {
        const unsigned char* wf = wsl + (long long)(t - ta) * FWb;
        const float* af = asl + (long long)(t - ta) * C;
        Pick best = {-kInf, kNoArc, 0, 0.f};
        if (t == nf - 1) {
          const int n = C * R;
          for (int base = 0; base < n; base += 64) {
            const int k = base + lane;
            fold_slice<BF16>(best, k < n, k, k / R, wf, af, t, s, b, a);
          }
        } else {
          if (a.stage_csr) {
            const int2 sq = seg[q];
            for (int base = 0; base < sq.y; base += 64) {
              const int j = base + lane;
              const bool ok = j < sq.y;
              const int2 kp = pair[sq.x + (ok ? j : 0)];
              fold_slice<BF16>(best, ok, kp.x, kp.y, wf, af, t, s, b, a);
            }
          } else {
            const int o0 = a.in_off[q];
            const int n = a.in_off[q + 1] - o0 + 1;
            for (int base = 0; base < n; base += 64) {
              const int j = base + lane;
              const bool ok = j < n;
              int k = q * R, p = q;  // candidate 0: the blank arc
              if (ok && j > 0) {
                const int id = a.in_arc[o0 + j - 1];
                p = id / a.V;
                k = p * R + (id - p * a.V) + 1;
              }
              fold_slice<BF16>(best, ok, k, p, wf, af, t, s, b, a);
            }
          }
        }
        // every candidate NaN (never for finite log_z): the blank arc
        if (best.k == kNoArc) {
          best.k = q * R;
          best.p = q;
          best.w = ldw<BF16>(wf, q * R);
        }
        q = best.p;
        wsum += best.w;
        if (lane == (t & 63)) lab = best.k - best.p * R;
        if ((t & 63) == 0) {
          if (t + lane < T) out[t + lane] = lab;
          lab = 0;
        }
      }
    }
    if constexpr (RING) {
      if (i + 1 < nsl) LT_SLICE_STORE(i + 1)
      __syncthreads();
    }
  }
  if (active && lane == 0) a.pw[(long long)b * a.S + s] = wsum;
}

struct SamplePlan {
  int wpb, nblk, threads;
  int L, capW, capA, stage_csr;
  int lds;
};

// Validates the shape and lays out the workgroup and its LDS.
int sample_plan(const lt_graph* g, const lt_table_problem* pb, int num_samples, SamplePlan* pl) {
  if (int rc = table_check("lt_table_sample", g, pb, 0, [&] {
        if (num_samples < 1) return fail(LT_EINVAL, "lt_table_sample: num_samples < 1");
        if (g->expansions >= 1)
          return fail(LT_EUNSUPPORTED, "lt_table_sample: FrameLabelDependent is not sampled");
        return check_arrays(g, true);
      }))
    return rc;
  const long long C = g->num_states, V = g->vocab_size, R = V + 1;
  pl->wpb = num_samples < 8 ? num_samples : 8;
  pl->nblk = (num_samples + pl->wpb - 1) / pl->wpb;
  if ((long long)pl->nblk * pb->batch > 0x7fffffffLL ||
      (long long)num_samples * pb->batch > 0x7fffffffLL)
    return fail(LT_EUNSUPPORTED, "lt_table_sample: 2^31 samples or more");
  pl->threads = 64 * (pl->wpb < 4 ? 4 : pl->wpb);
  // the ring: the most whole frames whose image, W and alpha each with up to
  // 15 bytes of misalignment in front, is kSampleKpt 16-byte loads a thread
  const long long es = pb->weight_dtype == LT_DTYPE_BF16 ? 2 : 4;
  const long long fw = C * R * es, fa = C * 4;
  const long long budget = (long long)pl->threads * kSampleKpt;
  auto chunks = [](long long bytes) { return ((bytes + 15) >> 4) + 1; };
  long long L = 0;
  while (L < pb->max_frames && L < 64 && chunks((L + 1) * fw) + chunks((L + 1) * fa) <= budget)
    ++L;
  pl->L = (int)L;
  pl->capW = L ? (int)chunks(L * fw) : 0;
  pl->capA = L ? (int)chunks(L * fa) : 0;
  const long long ring = 2LL * 16 * (pl->capW + pl->capA);
  const long long csr = 8 * C + 8 * (C * V + C);  // seg + pairs
  pl->stage_csr = csr <= kSampleCsr && ring + csr <= kTabLds ? 1 : 0;
  pl->lds = (int)(ring + (pl->stage_csr ? csr : 0));
  return LT_OK;
}

}  // namespace

extern "C" {

int lt_table_sample_workspace_bytes(const lt_graph* g, const lt_table_problem* pb,
                                    int32_t num_samples, size_t* bytes) {
  SamplePlan pl;
  if (int rc = sample_plan(g, pb, num_samples, &pl)) return rc;
  if (bytes) *bytes = 0;
  return LT_OK;
}

int lt_table_sample(const lt_graph* g, const lt_table_problem* pb, const void* W,
                    const int32_t* num_frames, const float* log_z, const float* alpha,
                    int32_t num_samples, uint64_t seed, int64_t* labels, float* path_weight,
                    void* workspace, size_t workspace_bytes, void* stream) {
  (void)workspace;
  (void)workspace_bytes;
  SamplePlan pl;
  if (int rc = sample_plan(g, pb, num_samples, &pl)) return rc;
  if (!path_weight || (!labels && pb->max_frames > 0))
    return fail(LT_EINVAL, "lt_table_sample: null output");
  if (pb->batch == 0) return LT_OK;
  if (!num_frames || !log_z || ((!W || !alpha) && pb->max_frames > 0))
    return fail(LT_EINVAL, "null pointer");
  if (((uintptr_t)W & 15) || ((uintptr_t)alpha & 15) || ((uintptr_t)num_frames & 3) ||
      ((uintptr_t)log_z & 3) || ((uintptr_t)labels & 7) || ((uintptr_t)path_weight & 3))
    return fail(LT_EINVAL, "misaligned pointer");
  SArgs a;
  memset(&a, 0, sizeof(a));
  a.W = (const unsigned char*)W;
  a.nfr = num_frames;
  a.logz = log_z;
  a.alpha = alpha;
  a.table = g->next_state;
  a.in_off = g->in_offsets;
  a.in_arc = g->in_arcs;
  a.out = (long long*)labels;
  a.pw = path_weight;
  a.key0 = (unsigned)(seed & 0xffffffffu);
  a.key1 = (unsigned)(seed >> 32);
  a.B = pb->batch;
  a.T = pb->max_frames;
  a.C = g->num_states;
  a.V = g->vocab_size;
  a.R = g->vocab_size + 1;
  a.S = num_samples;
  a.wpb = pl.wpb;
  a.nblk = pl.nblk;
  a.L = pl.L;
  a.capW = pl.capW;
  a.capA = pl.capA;
  a.stage_csr = pl.stage_csr;
  return dispatch(pb->weight_dtype == LT_DTYPE_BF16, [&](auto bf) {
    constexpr bool BF16 = decltype(bf)::value;
    auto k = a.L ? sample_kernel<BF16, true> : sample_kernel<BF16, false>;
    return launch(k, dim3((unsigned)(a.B * pl.nblk)), dim3(pl.threads), pl.lds,
                  (hipStream_t)stream, a, "sampling");
  });
}

}  // extern "C"
