// lt_align_long.hip -- the forced alignment of lt_align.hip for label strings
// of 256 <= U <= 4095 (include/lt_align_long.h): the same definition, tie
// rule and fp32 sums per position, the string split over the waves of one
// workgroup, forward and backtrace in ONE launch. FrameDependent only.
//
// One workgroup per utterance, NW = ceil((U+1)/256) waves (2 .. 16; the kernel
// is instantiated on NW, so its register budget and the depth of its weight
// ring follow the workgroup's size). Wave w holds positions 256w .. 256w+255,
// four consecutive ones a lane; alpha stays in registers.
//
//   own waves  Positions above num_labels never feed positions at or below
//              it: only the nwb = num_labels/256 + 1 lowest waves of an
//              utterance run the recursion, the others pass the barriers.
//   carry      Inside a wave position u-1 is one DPP lane shift away. Lane 0
//              of wave w needs, at frame t, alpha_t[256w-1] + lex_t[256w-1]:
//              the sum lane 63 of wave w-1 forms for its own shift at that
//              frame. It travels as that one rounded sum and becomes the fill
//              value of the receiving wave's shift.
//   pipeline   Frames are taken in blocks of kF. At block-step s wave w runs
//              block s-w, lane 63 writes the block's outgoing sums into an LDS
//              ring [NW-1][2][kF] of floats (double-buffered by block parity)
//              and wave w+1 reads them one block-step later, one per lane,
//              handing them out by v_readlane: no LDS read sits on the chain.
//              ONE __syncthreads() per block-step, none per frame:
//              ceil(nf/kF) + nwb - 1 of them, the same count in every wave.
//   decisions  One ballot per position slice: wave w stores four 64-bit words
//              a frame, word (t, w, j) bit l = position 256w + 4l + j took
//              its lexical term, in the caller's workspace [B, T, NW, 4].
//   backtrace  Thread 0 walks one bit per frame down from (nf, num_labels).
//              Within 256 frames the position drops by at most 256, so it
//              stays inside two waves' slices: per chunk of kChunk = 256
//              frames the walker publishes its position, the whole workgroup
//              stages those two waves' words of the chunk's frames (64 bytes a
//              frame) into LDS, and the walker reads whole staged rows, whose
//              addresses do not depend on the position, last chunk first. A
//              walk that has reached position 0 ends: the rows were filled
//              with 0 / -1 by the whole workgroup before the forward, which
//              is also the answer for an unaligned utterance.
// The weights of a frame do not depend on alpha: they are gathered kD frames
// ahead into a register ring that runs on across the blocks. No atomics.
#include "lt_string_common.h"

namespace {

constexpr int kF = 16;       // frames of a pipeline block
constexpr int kChunk = 256;  // frames staged per chunk of the backtrace (tests: CHUNK)
static_assert(kChunk <= 256, "a chunk's positions stay inside two waves' slices");

struct LaArgs {
  const unsigned char* W;
  const int* nfr;
  const int* table;    // [C, V] next state of (p, y)
  const int* labels;   // [B, U]
  const int* nlab;     // [B]
  long long* out;      // [B, T] alignment labels
  long long* frames;   // [B, U] frame of the arc leaving position u (nullable)
  float* dist;         // [B]
  unsigned long long* ws;  // decisions [B, T, NW, 4]
  int B, T, U, C, V, R;
  int stage_tab;       // the next-state table is staged in LDS for the walk
};

LT_DEVINL float lane_value(float x, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l));
}

// bytes of the carry ring and the two scalars behind it (the final alpha, the
// walker's position), rounded so that the staging band is 16-byte aligned
constexpr int ring_bytes(int NW) { return ((NW - 1) * 2 * kF * 4 + 8 + 15) & ~15; }
constexpr int kBandBytes = kChunk * 8 * 8;

template <bool BF16, int NW>
__global__ __launch_bounds__(64 * NW) void align_long_kernel(const LaArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char la_sm[];
  constexpr int P = 4, SPT = 256 * NW, NT = 64 * NW, F = kF;
  // frames of weights in flight: 8 D registers. Up to 8 waves a SIMD holds at
  // most two of them (256 VGPRs each), beyond that up to four (128)
  constexpr int D = NW <= 8 ? 16 : 8;
  static_assert(F % D == 0, "a block is whole rounds of the register ring");
  constexpr int ES = BF16 ? 2 : 4;
  const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int U = a.U, T = a.T;
  int nf = a.nfr[b];
  nf = nf < 0 ? 0 : (nf > T ? T : nf);

  // ---- outputs of an unaligned utterance; the backtrace overwrites its own
  long long* out = a.out + (long long)b * T;
  for (int i = tid; i < T; i += NT) out[i] = 0;
  long long* lfr = a.frames ? a.frames + (long long)b * U : nullptr;
  if (lfr)
    for (int i = tid; i < U; i += NT) lfr[i] = -1;
  const int nlb = a.nlab[b];
  if (nlb < 0 || nlb > U) {  // workgroup-uniform
    if (tid == 0) a.dist[b] = -kInf;
    return;
  }
  const int fin = nlb;
  const int nwb = (fin >> 8) + 1;  // the waves that hold positions 0 .. fin

  // ---- string positions: context state and label class
  int ob[P], ol[P];
  const StringLds sl = string_prologue<P, NT, 0, SPT>(a, b, tid, lane, la_sm, ob, ol, 256 * w);
  const int* yt = sl.yt;
  // the carry ring, two scalars and the staging band take the staged table's place
  float* ring = (float*)sl.region;
  float* fslot = ring + (NW - 1) * 2 * F;
  int* qslot = (int*)(fslot + 1);
  unsigned long long* band = (unsigned long long*)(sl.region + ring_bytes(NW));

  // ---- forward
  const long long FRB = (long long)a.C * a.R * ES;
  const unsigned char* wbase = a.W + (long long)b * T * FRB;
  unsigned long long* gdec = a.ws + (long long)b * T * (4 * NW);
  const bool run = w < nwb;
  const bool has_in = w > 0, has_out = w < nwb - 1;
  const float* rin = ring + (has_in ? w - 1 : 0) * 2 * F;
  float* rout = ring + (has_out ? w : 0) * 2 * F;
  float al[P];
#pragma unroll
  for (int j = 0; j < P; ++j) al[j] = (tid == 0 && j == 0) ? 0.f : -kInf;
  float pb[D][P], pl[D][P];
  if (run && nf > 0) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const unsigned char* wf = wbase + (long long)(d < nf ? d : nf - 1) * FRB;
#pragma unroll
      for (int j = 0; j < P; ++j) {
        pb[d][j] = ldw<BF16>(wf, ob[j]);
        pl[d][j] = ldw<BF16>(wf, ol[j]);
      }
    }
  }
  const int nb = (nf + F - 1) / F;
  const int nsteps = nb ? nb + nwb - 1 : 0;
  for (int s = 0; s < nsteps; ++s) {
    const int k = s - w;
    const int ib = k * F;
    if (run && k >= 0 && ib < nf) {
      // the block's incoming carries, frame f in lane f
      float cin = -kInf;
      if (has_in && lane < F) cin = rin[(k & 1) * F + lane];
      float* co = rout + (k & 1) * F;
      for (int h = 0; h < F; h += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
          const int f = h + d, t = ib + f;
          if (t >= nf) break;
          float wb[P], wl[P];
#pragma unroll
          for (int j = 0; j < P; ++j) {
            wb[j] = pb[d][j];
            wl[j] = pl[d][j];
          }
          {
            const int tn = t + D < nf ? t + D : nf - 1;
            const unsigned char* wf = wbase + (long long)tn * FRB;
#pragma unroll
            for (int j = 0; j < P; ++j) {
              pb[d][j] = ldw<BF16>(wf, ob[j]);
              pl[d][j] = ldw<BF16>(wf, ol[j]);
            }
          }
          float lo[P];
#pragma unroll
          for (int j = 0; j < P; ++j) lo[j] = al[j] + wl[j];
          // what the next wave's shift takes in at this frame
          if (has_out && lane == 63) co[f] = lo[P - 1];
          const float up = wave_prev(lo[P - 1], lane_value(cin, f));
          unsigned long long m[P];
#pragma unroll
          for (int j = 0; j < P; ++j) {
            const float x = al[j] + wb[j];
            const float y = j ? lo[j ? j - 1 : 0] : up;
            const bool ge = x >= y;
            // position 0 has no lexical term: a NaN blank term ends the path there
            const bool lex = !ge && !(tid == 0 && j == 0);
            al[j] = ge ? x : y;
            m[j] = __ballot(lex);
          }
          // lane j keeps word j of the wave's frame
          unsigned long long mine = m[0];
#pragma unroll
          for (int j = 1; j < P; ++j) mine = lane == j ? m[j] : mine;
          if (lane < P) gdec[((long long)t * NW + w) * P + lane] = mine;
        }
      }
    }
    __syncthreads();  // the block's carries
  }

  // ---- alpha_nf at num_labels: one lane has it, every wave needs it
  if (tid == (fin >> 2)) {
    float mine = al[0];
#pragma unroll
    for (int j = 1; j < P; ++j) mine = (fin & 3) == j ? al[j] : mine;
    *fslot = mine;
  }
  __syncthreads();  // and the rows' fill and the decisions, before thread 0's stores / loads
  const float fv = *fslot;
  if (tid == 0) a.dist[b] = fv;
  if (!(fv > -kInf)) return;  // unaligned (workgroup-uniform)

  // ---- backtrace: chunks of kChunk frames, the last first
  int q = fin;
  for (int t1 = nf; t1 > 0; t1 -= kChunk) {
    const int t0 = t1 - kChunk > 0 ? t1 - kChunk : 0;
    if (tid == 0) *qslot = q;
    __syncthreads();  // the position; the walker is done with the last chunk's band
    const int qs = *qslot;
    if (qs == 0) break;  // only blank arcs are left (workgroup-uniform)
    // the chunk's positions are in (qs - 256, qs]: the slices of two waves
    const int wq = qs >> 8;
    const int wlo = wq > 0 ? wq - 1 : 0, whi = wq > 0 ? wq : 0;
    for (int i = tid; i < (t1 - t0) * 8; i += NT) {
      const int f = i >> 3, c = i & 7;
      band[i] = gdec[((long long)(t0 + f) * NW + (c < 4 ? wlo : whi)) * P + (c & 3)];
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll 4
      for (int t = t1 - 1; t >= t0; --t) {
        // the whole row: its address does not depend on q
        const unsigned long long* row = band + (t - t0) * 8;
        const int c0 = (q >> 8) != wlo ? 4 : 0;
        unsigned long long wd = row[0];
#pragma unroll
        for (int c = 1; c < 8; ++c) wd = (c0 + (q & 3)) == c ? row[c] : wd;
        const int d = q > 0 ? (int)((wd >> ((q & 255) >> 2)) & 1) : 0;
        if (d) {
          --q;
          out[t] = yt[q];
          if (lfr) lfr[q] = t;
        }
      }
    }
  }
}

struct LongAlignPlan {
  int NW, stage_tab, lds;
  size_t ws;
};

// Validates the shape and lays out LDS / workspace.
int long_align_plan(const lt_graph* g, const lt_table_problem* pb, LongAlignPlan* pl) {
  if (int rc = table_check("lt_table_align_long", g, pb, kChkString, [&] {
        if (g->expansions > 0)
          return fail(LT_EUNSUPPORTED, "lt_table_align_long: FrameLabelDependent (expansions >= 1)");
        if (pb->max_labels < 256 || pb->max_labels > 4095)
          return fail(LT_EUNSUPPORTED, "lt_table_align_long: max_labels outside 256..4095");
        return LT_OK;
      }))
    return rc;
  pl->NW = (pb->max_labels + 256) / 256;
  const long long stage = stage_table(g);
  pl->stage_tab = stage ? 1 : 0;
  // ctx, yn, yt; then the staged table, and in its place the ring and the band
  const long long after = ring_bytes(pl->NW) + kBandBytes;
  const long long lds = 3LL * 4 * 256 * pl->NW + ((std::max(stage, after) + 15) & ~15LL);
  if (lds > kTabLds) return fail(LT_EUNSUPPORTED, "lt_table_align_long: the LDS layout does not fit");
  pl->lds = (int)lds;
  // a frame of decisions is four 64-bit words a wave
  pl->ws = (size_t)(((long long)pb->batch * pb->max_frames * 32 * pl->NW + 255) & ~255LL);
  return LT_OK;
}

// the launch of the kernel instantiated on nw waves (2 .. 16)
template <bool BF16, int NW = 2>
int launch_waves(int nw, int lds, hipStream_t st, const LaArgs& a) {
  if constexpr (NW > 16) {
    return fail(LT_EUNSUPPORTED, "lt_table_align_long: max_labels outside 256..4095");
  } else {
    if (nw == NW)
      return launch(align_long_kernel<BF16, NW>, dim3(a.B), dim3(64 * NW), lds, st, a,
                    "long alignment");
    return launch_waves<BF16, NW + 1>(nw, lds, st, a);
  }
}

}  // namespace

extern "C" {

int lt_table_align_long_workspace_bytes(const lt_graph* g, const lt_table_problem* pb,
                                        size_t* bytes) {
  LongAlignPlan pl;
  if (int rc = long_align_plan(g, pb, &pl)) return rc;
  if (bytes) *bytes = pl.ws;
  return LT_OK;
}

int lt_table_align_long(const lt_graph* g, const lt_table_problem* pb, const void* W,
                        const int32_t* num_frames, const int32_t* labels,
                        const int32_t* num_labels, int64_t* alignment_labels,
                        int64_t* label_frames, float* path_weight, void* workspace,
                        size_t workspace_bytes, void* stream) {
  LongAlignPlan pl;
  if (int rc = long_align_plan(g, pb, &pl)) return rc;
  if (pb->batch == 0) return LT_OK;
  if ((!W && pb->max_frames > 0) || !num_frames || !num_labels || !path_weight ||
      (!alignment_labels && pb->max_frames > 0) || !labels)
    return fail(LT_EINVAL, "null pointer");
  const bool bf16 = pb->weight_dtype == LT_DTYPE_BF16;
  if (((uintptr_t)W & (bf16 ? 1 : 3)) || ((uintptr_t)num_frames & 3) || ((uintptr_t)labels & 3) ||
      ((uintptr_t)num_labels & 3) || ((uintptr_t)alignment_labels & 7) ||
      ((uintptr_t)label_frames & 7) || ((uintptr_t)path_weight & 3) || ((uintptr_t)workspace & 7))
    return fail(LT_EINVAL, "misaligned pointer");
  if (pl.ws && (!workspace || workspace_bytes < pl.ws))
    return fail(LT_EINVAL, "workspace too small");
  LaArgs a;
  memset(&a, 0, sizeof(a));
  a.W = (const unsigned char*)W;
  a.nfr = num_frames;
  a.table = g->next_state;
  a.labels = labels;
  a.nlab = num_labels;
  a.out = (long long*)alignment_labels;
  a.frames = (long long*)label_frames;
  a.dist = path_weight;
  a.ws = (unsigned long long*)workspace;
  a.B = pb->batch;
  a.T = pb->max_frames;
  a.U = pb->max_labels;
  a.C = g->num_states;
  a.V = g->vocab_size;
  a.R = g->vocab_size + 1;
  a.stage_tab = pl.stage_tab;
  hipStream_t st = (hipStream_t)stream;
  return dispatch(bf16, [&](auto bf) {
    return launch_waves<decltype(bf)::value>(pl.NW, pl.lds, st, a);
  });
}

}  // extern "C"
