// lt_beam.hip -- prefix beam search over the denominator lattice (any
// next-state table x FrameDependent): the K best label sequences, each scored
// by the (+)-sum of its kept alignments. The search is specified in
// include/lt_beam.h (candidates, the merge of a prefix with its parent's
// extension, the total order of the selection, the prefix hash), so the beams
// do not depend on the launch.
//
// One workgroup per utterance; its wave 0 searches, lane r is slot r, and the
// slot state (score, context state, length, hash, parent hash, last label)
// lives in registers. The other waves only stage.
//   ring      the frames are visited in order, only the rows inside a frame
//             depend on the beam. The workgroup stages whole frames of W one
//             slice of L frames ahead into a two-slice LDS ring: 16-byte
//             loads issued before a slice is searched, written to the other
//             half after it, one barrier a slice.
//   no ring   a frame larger than a slice (32 KiB) is gathered from memory,
//             row by row; the workgroup is then the one wave.
//   merge     one pass over the live slots j: v_readlane broadcasts slot j,
//             and every lane i asks both "is j my parent?" (it keeps j's score
//             and state, and afterwards adds cand(j, y_i) into its blank
//             candidate) and "is j my child?" (it sets bit y_j of its own
//             mask row in LDS: R bits a slot, bit y = candidate (slot, y) is
//             removed or taken). Each lane then publishes its slot's (score,
//             state, merged blank candidate) in LDS.
//   select    the live slots' candidates k = slot*R + label are dealt
//             round-robin to the 64 lanes (lane l: k = l, l + 64, ...), so a
//             narrow beam still uses the whole wave and the candidates of one
//             strong slot land on different lanes. A lane scores its share
//             once, four gathers in flight, and keeps its four best, sorted,
//             in registers. K rounds of a DPP wave max over the 64 lane bests
//             and a ballot (equal scores: the smallest k, by v_readlane);
//             the winning lane sets the candidate's mask bit and pops its
//             list, and scores its share again only when the four are used
//             up and it holds more. Lane r keeps round r's (source, label,
//             score); after the rounds every lane fetches its source's state
//             by ds_bpermute into fresh registers, so no new slot is written
//             while an old one is still read.
//   trace     lane r stores (source << 16) | label of frame t, coalesced. After
//             the last frame, behind a device-scope fence, lane r walks its
//             chain back from frame nf-1 and writes its labels back to front.
#include "lt_string_common.h"

namespace {

struct BArgs {
  const unsigned char* W;
  const int* nfr;
  const int* table;   // [C, V] next state of (p, y)
  long long* labels;  // [B, K, T]
  int* nlab;          // [B, K]
  float* scores;      // [B, K]
  int* trace;         // [B, T, K] (the caller's, or the workspace)
  float* step;        // [B, T, K] or null
  int pad_trace;      // the padding frames of `trace` are an output
  int B, T, C, V, R, K;
  int L;          // frames per ring slice (0: no ring)
  int capW;       // 16-byte chunks of a slice's image
  int MW;         // 32-bit words of a slot's removed-label mask
  int stage_tab;  // the next-state table is staged in LDS
};

constexpr int kBeamKpt = 4;             // 16-byte loads a thread holds per slice
constexpr int kBeamThreads = 512;       // workgroup of the ring kernel
constexpr int kBeamMaxK = 64;
constexpr int kBeamMaxV = 1023;

LT_DEVINL unsigned long long readlane64(unsigned long long v, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}
LT_DEVINL unsigned long long shfl64(unsigned long long v, int l) {
  const unsigned lo = (unsigned)__shfl((int)(unsigned)v, l);
  const unsigned hi = (unsigned)__shfl((int)(unsigned)(v >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}

// the hash of prefix + y (include/lt_beam.h)
LT_DEVINL unsigned long long mix(unsigned long long h, int y) {
  unsigned long long z = h ^ ((unsigned long long)y * 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// a candidate: one fp32 add, NaN counts as -inf
LT_DEVINL float cand(float s, float w) {
  const float v = s + w;
  return v == v ? v : -kInf;
}

// The ring's slice i of an utterance: frames [i*L, min(nf, (i+1)*L)), as a
// byte range widened to whole 16-byte granules.
struct SliceGeom {
  const unsigned char* w;  // the utterance's W
  long long fw;            // bytes of a frame
  int nf, L;
};
struct SliceRange {
  unsigned long long gw;  // 16-byte aligned start
  int nW;                 // granules
};
LT_DEVINL SliceRange slice_range(const SliceGeom& g, int i) {
  const int ta = i * g.L, tb = ta + g.L < g.nf ? ta + g.L : g.nf;
  const unsigned long long gw = (unsigned long long)(g.w + (long long)ta * g.fw);
  SliceRange r;
  r.nW = (int)(((gw & 15) + (unsigned long long)(tb - ta) * g.fw + 15) >> 4);
  r.gw = gw & ~15ull;
  return r;
}
// granule j of the slice (granules past it repeat its first one: always in
// range, never stored)
LT_DEVINL uint4 granule_load(const SliceRange& r, int j) {
  return *(const uint4*)(j < r.nW ? r.gw + 16ull * j : r.gw);
}
LT_DEVINL void granule_store(const SliceRange& r, int j, unsigned char* buf, const uint4& v) {
  if (j < r.nW) *(uint4*)(buf + 16 * j) = v;
}
// thread tid holds granules tid + k*NT, k < kBeamKpt = 4, in four registers
#define LT_BEAM_LOAD(i)                       \
  {                                           \
    const SliceRange r_ = slice_range(sg, (i)); \
    rg0 = granule_load(r_, tid);              \
    rg1 = granule_load(r_, tid + NT);         \
    rg2 = granule_load(r_, tid + 2 * NT);     \
    rg3 = granule_load(r_, tid + 3 * NT);     \
  }
#define LT_BEAM_STORE(i)                                  \
  {                                                       \
    const SliceRange r_ = slice_range(sg, (i));           \
    unsigned char* buf_ = s_sm + ((i) & 1) * sliceB;      \
    granule_store(r_, tid, buf_, rg0);                    \
    granule_store(r_, tid + NT, buf_, rg1);               \
    granule_store(r_, tid + 2 * NT, buf_, rg2);           \
    granule_store(r_, tid + 3 * NT, buf_, rg3);           \
  }
static_assert(kBeamKpt == 4, "LT_BEAM_LOAD / LT_BEAM_STORE hold four granules");

// The slot state of the searching wave: lane r is slot r.
struct Slot {
  float s;                    // score; -inf: dead
  int c, n, y;                // context state, length, last label
  unsigned long long h, ph;   // hash of the prefix, of its parent
};

// Lane l's first candidate k = l as (slot, label) = (l / R, l % R), and the
// step of k += 64.
struct LaneDeal {
  int i0, y0, di, dy;
};

// One frame of the search (wave 0, all 64 lanes active). wf: the frame's W
// [C, R]; mrows: the slots' mask rows in LDS, MW words each (bit y: candidate
// (slot, y) is removed or taken); sbuf: the slots' (score, state, blank
// candidate) in LDS; tbl: the table.
template <int MODE, bool BF16>
LT_DEVINL void beam_frame(Slot& q, int& nlive, const unsigned char* wf, unsigned* mrows,
                          float4* sbuf, const int* tbl, const BArgs& a, const LaneDeal& ld,
                          int lane, long long tro) {
  constexpr int ES = BF16 ? 2 : 4;
  const int R = a.R, MW = a.MW;
  unsigned* mask = mrows + lane * MW;  // this slot's row
  const bool live = lane < nlive;
  const unsigned char* row = wf + (long long)q.c * R * ES;
  float cb = live ? cand(q.s, ldw<BF16>(row, 0)) : -kInf;
  for (int w = 0; w < MW; ++w) mask[w] = 0;
  // ---- merge
  bool hasp = false;
  float ps = 0.f;
  int pc = 0;
  for (int j = 0; j < nlive; ++j) {
    const unsigned long long hj = readlane64(q.h, j), phj = readlane64(q.ph, j);
    const int nj = __builtin_amdgcn_readlane(q.n, j), yj = __builtin_amdgcn_readlane(q.y, j);
    const int cj = __builtin_amdgcn_readlane(q.c, j);
    const float sj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(q.s), j));
    if (live && !hasp && q.n >= 1 && hj == q.ph && nj == q.n - 1) {  // j is my parent
      hasp = true;
      ps = sj;
      pc = cj;
    }
    if (live && nj >= 1 && phj == q.h && nj - 1 == q.n)  // j is my child
      mask[yj >> 5] |= 1u << (yj & 31);
  }
  if (hasp) {
    const float e = cand(ps, ldw<BF16>(wf + (long long)pc * R * ES, q.y));
    cb = MODE == M_LOG ? log_plus(cb, e) : (cb >= e ? cb : e);
    if (!(cb == cb)) cb = -kInf;
  }
  // ---- select: the candidates dealt round-robin to the 64 lanes, each
  // lane's four best in registers, then K rounds over the wave
  sbuf[lane] = make_float4(q.s, __int_as_float(q.c), cb, 0.f);
  float s0, s1, s2, s3;  // this lane's best candidates not yet taken, best first
  int p0, p1, p2, p3;    // as (slot << 16) | label: ordered as k = slot*R + label
  int nfin, wins;        // finite candidates the last scan saw; taken since
  auto insert = [&](float v, int p) {
    if (!(v > -kInf)) return;  // -inf and NaN are no candidates
    ++nfin;
    // after every element >= v: equal scores keep the scan's order, ascending k
    // (g0 implies g1 implies g2 implies g3, so the displaced one moves down)
    const bool g0 = v > s0, g1 = v > s1, g2 = v > s2, g3 = v > s3;
    float cs = v, ts;
    int cp = p, tp;
#define LT_BEAM_STAGE(G, S, P) \
  ts = S; tp = P;              \
  S = G ? cs : ts; P = G ? cp : tp; \
  cs = G ? ts : cs; cp = G ? tp : cp;
    LT_BEAM_STAGE(g0, s0, p0)
    LT_BEAM_STAGE(g1, s1, p1)
    LT_BEAM_STAGE(g2, s2, p2)
    LT_BEAM_STAGE(g3, s3, p3)
#undef LT_BEAM_STAGE
  };
  const int N = nlive * R;  // candidates k = slot*R + label; lane l has k = l, l + 64, ...
  auto scan = [&]() {
    s0 = s1 = s2 = s3 = -kInf;
    p0 = p1 = p2 = p3 = 0;
    nfin = wins = 0;
    int i = ld.i0, y = ld.y0;
    for (int k = lane; k < N;) {  // four candidates in flight
      float v[4];
      int p[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool ok = k < N;
        const int ii = ok ? i : 0, yy = ok ? y : 0;
        const float4 sl = sbuf[ii];  // (score, state, merged blank candidate)
        const unsigned m = mrows[ii * MW + (yy >> 5)];
        const float w = ldw<BF16>(wf + (long long)__float_as_int(sl.y) * R * ES, yy);
        const bool gone = (m >> (yy & 31)) & 1;  // removed by the merge, or taken
        v[u] = ok && !gone ? (yy == 0 ? sl.z : sl.x + w) : -kInf;
        p[u] = (ii << 16) | yy;
        k += 64;
        i += ld.di;
        y += ld.dy;
        if (y >= R) {
          y -= R;
          ++i;
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) insert(v[u], p[u]);
    }
  };
  scan();
  float ns = -kInf;
  int np = 0, nnew = 0;
  for (int r = 0; r < a.K; ++r) {
    const float top = wave_max(s0);
    if (!(top > -kInf)) break;  // no candidate left
    unsigned long long m = __ballot(s0 == top);
    int src = __ffsll((long long)m) - 1;
    int pw = __builtin_amdgcn_readlane(p0, src);
    for (m &= m - 1; m; m &= m - 1) {  // equal scores (rare): the smallest k
      const int l = __ffsll((long long)m) - 1;
      const int pl = __builtin_amdgcn_readlane(p0, l);
      if (pl < pw) {
        pw = pl;
        src = l;
      }
    }
    if (lane == r) {
      ns = top;
      np = pw;
    }
    if (lane == src) {
      mrows[(pw >> 16) * MW + ((pw & 0xffff) >> 5)] |= 1u << (pw & 31);  // taken
      s0 = s1; p0 = p1;
      s1 = s2; p1 = p2;
      s2 = s3; p2 = p3;
      s3 = -kInf; p3 = 0;
      ++wins;
      // the four are used up and the lane holds more: the taken ones are in
      // the masks, scan again
      if (!(s0 > -kInf) && wins < nfin) scan();
    }
    nnew = r + 1;
  }
  const int nsrc = np >> 16, nyw = np & 0xffff;
  // ---- the new beam, from the old one through ds_bpermute
  const unsigned long long sh = shfl64(q.h, nsrc), sph = shfl64(q.ph, nsrc);
  const int sn = __shfl(q.n, nsrc), sc = __shfl(q.c, nsrc), sy = __shfl(q.y, nsrc);
  const bool kept = lane < nnew;
  Slot z = {-kInf, 0, 0, 0, 0ull, 0ull};
  if (kept) {
    z.s = ns;
    if (nyw == 0) {
      z.c = sc; z.n = sn; z.y = sy; z.h = sh; z.ph = sph;
    } else {
      z.c = tbl[(long long)sc * a.V + nyw - 1];
      z.n = sn + 1;
      z.y = nyw;
      z.h = mix(sh, nyw);
      z.ph = sh;
    }
  }
  q = z;
  nlive = nnew;
  if (lane < a.K) {
    a.trace[tro + lane] = kept ? (nsrc << 16) | nyw : -1;
    if (a.step) a.step[tro + lane] = kept ? ns : -kInf;
  }
}

template <int MODE, bool BF16, bool RING>
__global__ __launch_bounds__(RING ? kBeamThreads : 64) void beam_kernel(const BArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_sm[];
  constexpr int ES = BF16 ? 2 : 4;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int NT = blockDim.x;
  const int b = blockIdx.x;
  const int T = a.T, K = a.K;
  int nf = a.nfr[b];
  nf = nf < 0 ? 0 : (nf > T ? T : nf);

  const int sliceB = RING ? 16 * a.capW : 0;
  unsigned* mrows = (unsigned*)(s_sm + 2 * sliceB);                  // [64, MW]
  float4* sbuf = (float4*)(s_sm + 2 * sliceB + 64 * a.MW * 4);       // [64]
  int* tab = (int*)(s_sm + 2 * sliceB + 64 * a.MW * 4 + 64 * 16);
  const LaneDeal ld = {lane / a.R, lane % a.R, 64 / a.R, 64 % a.R};
  if (a.stage_tab)
    for (int i = tid; i < a.C * a.V; i += NT) tab[i] = a.table[i];
  const int* tbl = a.stage_tab ? tab : a.table;

  // padding frames of the trace outputs
  const long long tr0 = (long long)b * T * K;
  for (long long i = (long long)nf * K + tid; i < (long long)T * K; i += NT) {
    if (a.pad_trace) a.trace[tr0 + i] = -1;
    if (a.step) a.step[tr0 + i] = -kInf;
  }

  const long long FWb = (long long)a.C * a.R * ES;  // bytes of a frame of W
  const unsigned char* wutt = a.W + (long long)b * T * FWb;

  uint4 rg0 = {}, rg1 = {}, rg2 = {}, rg3 = {};
  const SliceGeom sg = {wutt, FWb, nf, a.L};
  const int nsl = RING ? (nf + a.L - 1) / a.L : (nf > 0 ? 1 : 0);
  if constexpr (RING) {
    if (nsl > 0) {
      LT_BEAM_LOAD(0)
      LT_BEAM_STORE(0)
    }
  }
  __syncthreads();

  Slot q = {lane == 0 ? 0.f : -kInf, 0, 0, 0, 0ull, 0ull};
  int nlive = 1;
  for (int i = 0; i < nsl; ++i) {
    const int ta = RING ? i * a.L : 0;
    const int tb = RING ? (ta + a.L < nf ? ta + a.L : nf) : nf;
    if constexpr (RING)
      if (i + 1 < nsl) LT_BEAM_LOAD(i + 1)
    if (wave == 0) {
      const unsigned char* wsl;
      if constexpr (RING) {
        const unsigned long long gw = (unsigned long long)(wutt + (long long)ta * FWb);
        wsl = s_sm + (i & 1) * sliceB + (gw & 15);
      } else {
        wsl = wutt;
      }
      for (int t = ta; t < tb; ++t)
        beam_frame<MODE, BF16>(q, nlive, wsl + (long long)(t - ta) * FWb, mrows, sbuf, tbl, a, ld,
                               lane, tr0 + (long long)t * K);
    }
    if constexpr (RING) {
      if (i + 1 < nsl) LT_BEAM_STORE(i + 1)
      __syncthreads();
    }
  }
  if (wave != 0) return;

  // ---- outputs: scores, lengths, the zeros behind each label sequence
  if (lane < K) {
    a.scores[(long long)b * K + lane] = q.s;
    a.nlab[(long long)b * K + lane] = q.n;
  }
  long long* out = a.labels + (long long)b * K * T;
  for (int k = 0; k < K; ++k) {
    const int nk = __builtin_amdgcn_readlane(q.n, k);
    for (int p = nk + lane; p < T; p += 64) out[(long long)k * T + p] = 0;
  }
  // ---- backtrace: the trace rows were stored by other lanes of this wave
  __threadfence();
  if (lane < nlive) {
    int cur = lane, pos = q.n;
    for (int t = nf - 1; t >= 0 && pos > 0; --t) {
      const int e = a.trace[tr0 + (long long)t * K + cur];
      if (e < 0) break;
      const int y = e & 0xffff;
      if (y) out[(long long)lane * T + --pos] = y;
      cur = e >> 16;
    }
  }
}

struct BeamPlan {
  int threads, L, capW, MW, stage_tab, lds;
  size_t trace_bytes;
};

// Validates the shape and lays out the workgroup and its LDS.
int beam_plan(const lt_graph* g, const lt_table_problem* pb, int beam_size, BeamPlan* pl) {
  if (int rc = table_check("lt_table_beam_search", g, pb, 0, [&] {
        if (beam_size < 1) return fail(LT_EINVAL, "lt_table_beam_search: beam_size < 1");
        if (g->expansions >= 1)
          return fail(LT_EUNSUPPORTED, "lt_table_beam_search: FrameLabelDependent is not searched");
        if (int rc = check_arrays(g, false)) return rc;
        if (beam_size > kBeamMaxK)
          return fail(LT_EUNSUPPORTED, "lt_table_beam_search: beam_size > 64 (one wave)");
        if (g->vocab_size > kBeamMaxV)
          return fail(LT_EUNSUPPORTED, "lt_table_beam_search: V > 1023");
        return LT_OK;
      }))
    return rc;
  const long long C = g->num_states, R = g->vocab_size + 1;
  const long long ntrace = (long long)pb->batch * pb->max_frames * beam_size;
  if (ntrace > 0x7fffffffLL)
    return fail(LT_EUNSUPPORTED, "lt_table_beam_search: a trace of 2^31 elements or more");
  pl->trace_bytes = (size_t)ntrace * 4;
  // the ring: the most whole frames whose image, with up to 15 bytes of
  // misalignment in front, is kBeamKpt 16-byte loads a thread
  const long long es = pb->weight_dtype == LT_DTYPE_BF16 ? 2 : 4;
  const long long fw = C * R * es;
  const long long budget = (long long)kBeamThreads * kBeamKpt;
  auto chunks = [](long long bytes) { return ((bytes + 15) >> 4) + 1; };
  long long L = 0;
  while (L < pb->max_frames && L < 64 && chunks((L + 1) * fw) <= budget) ++L;
  pl->L = (int)L;
  pl->capW = L ? (int)chunks(L * fw) : 0;
  pl->threads = L ? kBeamThreads : 64;
  pl->MW = (int)((R + 31) / 32);
  const long long tabb = stage_table(g);
  pl->stage_tab = tabb ? 1 : 0;
  pl->lds = 2 * 16 * pl->capW + 64 * pl->MW * 4 + 64 * 16 + (int)tabb;
  return LT_OK;
}

}  // namespace

extern "C" {

int lt_table_beam_search_workspace_bytes(const lt_graph* g, const lt_table_problem* pb,
                                         int32_t beam_size, size_t* bytes) {
  BeamPlan pl;
  if (int rc = beam_plan(g, pb, beam_size, &pl)) return rc;
  if (bytes) *bytes = pl.trace_bytes;
  return LT_OK;
}

int lt_table_beam_search(const lt_graph* g, const lt_table_problem* pb, const void* W,
                         const int32_t* num_frames, int32_t beam_size, int32_t semiring,
                         int64_t* labels, int32_t* num_labels, float* scores, int32_t* trace,
                         float* step_score, void* workspace, size_t workspace_bytes,
                         void* stream) {
  BeamPlan pl;
  if (int rc = beam_plan(g, pb, beam_size, &pl)) return rc;
  if (semiring != LT_SEMIRING_LOG && semiring != LT_SEMIRING_MAX)
    return fail(LT_EINVAL, "lt_table_beam_search: the semiring is Log or MaxTropical");
  if (!num_labels || !scores || (!labels && pb->max_frames > 0))
    return fail(LT_EINVAL, "lt_table_beam_search: null output");
  if (pb->batch == 0) return LT_OK;
  if (!num_frames || (!W && pb->max_frames > 0)) return fail(LT_EINVAL, "null pointer");
  if (!trace && pl.trace_bytes > 0 && (!workspace || workspace_bytes < pl.trace_bytes))
    return fail(LT_EINVAL, "lt_table_beam_search: workspace too small for a null trace");
  if (((uintptr_t)W & 15) || ((uintptr_t)num_frames & 3) || ((uintptr_t)labels & 7) ||
      ((uintptr_t)num_labels & 3) || ((uintptr_t)scores & 3) || ((uintptr_t)trace & 3) ||
      ((uintptr_t)step_score & 3) || ((uintptr_t)workspace & 3))
    return fail(LT_EINVAL, "misaligned pointer");
  BArgs a;
  memset(&a, 0, sizeof(a));
  a.W = (const unsigned char*)W;
  a.nfr = num_frames;
  a.table = g->next_state;
  a.labels = (long long*)labels;
  a.nlab = num_labels;
  a.scores = scores;
  a.trace = trace ? trace : (int*)workspace;
  a.pad_trace = trace ? 1 : 0;
  a.step = step_score;
  a.B = pb->batch;
  a.T = pb->max_frames;
  a.C = g->num_states;
  a.V = g->vocab_size;
  a.R = g->vocab_size + 1;
  a.K = beam_size;
  a.L = pl.L;
  a.capW = pl.capW;
  a.MW = pl.MW;
  a.stage_tab = pl.stage_tab;
  return dispatch(pb->weight_dtype == LT_DTYPE_BF16, [&](auto bf) {
    constexpr bool BF16 = decltype(bf)::value;
    auto k = semiring == LT_SEMIRING_LOG
                 ? (a.L ? beam_kernel<M_LOG, BF16, true> : beam_kernel<M_LOG, BF16, false>)
                 : (a.L ? beam_kernel<M_MAX, BF16, true> : beam_kernel<M_MAX, BF16, false>);
    return launch(k, dim3((unsigned)a.B), dim3(pl.threads), pl.lds, (hipStream_t)stream, a,
                  "beam search");
  });
}

}  // extern "C"
