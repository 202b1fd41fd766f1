// lt_beam.hip -- prefix beam search over the denominator lattice (any
// next-state table x FrameDependent): the K best label sequences, each scored
// by the (+)-sum of its kept alignments. The search is specified in
// include/lt_beam.h (candidates, the merge of a prefix with its parent's
// extension, the total order of the selection, the prefix hash), so the beams
// do not depend on the launch.
//
// One workgroup per utterance; its wave 0 searches, lane r is slot r, and the
// slot state (score, context state, length, hash, parent hash, last label)
// lives in registers. The other waves only stage. The frame step (merge,
// select, trace) and the outputs are lt_beam_common.h's, shared with the fused
// joint search of lt_beam_joint.hip.
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
#include "lt_beam_common.h"

namespace {

constexpr int kBeamKpt = 4;             // 16-byte loads a thread holds per slice
constexpr int kBeamThreads = 512;       // workgroup of the ring kernel

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
        beam_frame<MODE, BF16, false>(q, nlive, wsl + (long long)(t - ta) * FWb, mrows, sbuf, tbl,
                                      a, ld, lane, tr0 + (long long)t * K);
    }
    if constexpr (RING) {
      if (i + 1 < nsl) LT_BEAM_STORE(i + 1)
      __syncthreads();
    }
  }
  if (wave == 0) beam_finish(q, nlive, a, b, nf, lane, tr0);
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
