// lt_align.hip -- forced alignment of label strings: the MaxTropical best
// path of the lattice intersected with the label string (the string acceptor
// of RecognitionLattice._string_forward, lattices.py:250-377, through
// FrameDependent.string_forward alignments.py:320-329 or
// FrameLabelDependent.string_forward :420-432), forward and backtrace in ONE
// launch, for any next-state table.
//
// One wave (one 64-thread workgroup) per utterance; no wave waits for another.
//   prologue   string_prologue (lt_string_common.h): labels to LDS, one lane
//              walks the context states (the table staged in LDS while it is
//              small), every lane keeps the two weight offsets of its
//              P = ceil((U+1)/64) consecutive string positions in registers
//   forward    alpha in registers; a frame is P adds per term, one DPP wave
//              shift of each lane's top position to its neighbour and one
//              ballot per position slice: the winning term of (t, u) is one
//              bit (FrameLabelDependent: ceil(log2(K+1)) bit planes) of a
//              64-bit word per frame and slice. The weights of a frame do
//              not depend on alpha: they are loaded kD frames ahead.
//   decisions  in LDS while T frames of them fit beside the prologue's
//              arrays (160 KiB per workgroup), else in the caller's
//              workspace, staged back in chunks of whole frames
//   backtrace  lane 0 walks one bit (plane set) per frame from num_labels
//              and stores the at most U labels / frames it meets; the rows
//              were filled with 0 / -1 by the whole wave before the forward
// Tie rules and arithmetic are tab_str_grad_kernel's (lt_table.hip) and
// table_oracle.c frame_max's: FrameDependent takes the blank term when
// x >= y, FrameLabelDependent the smallest expansion count; fp32 sums in the
// same order, so the path weight is bit-equal to lt_table_num_forward's.
#include "lt_string_common.h"

namespace {

struct AArgs {
  const unsigned char* W;
  const int* nfr;
  const int* table;    // [C, V] next state of (p, y)
  const int* labels;   // [B, U]
  const int* nlab;     // [B]
  long long* out;      // [B, T*A] alignment labels
  long long* frames;   // [B, U] frame of the arc leaving position u (nullable)
  float* dist;         // [B]
  unsigned long long* ws;  // decisions [B, T, planes*P] when they do not fit LDS
  int B, T, U, C, V, R, K;
  int planes;     // bit planes per decision (1 for FrameDependent)
  int dec_lds;    // decisions live in LDS
  int stage_tab;  // the next-state table is staged in LDS for the walk
  int chunk;      // frames staged per chunk of the backtrace (!dec_lds)
};

constexpr int kAlignChunk = 32 * 1024;  // bytes of decisions staged per chunk

template <bool BF16, int P, bool FLD>
__global__ __launch_bounds__(64) void align_kernel(const AArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char a_sm[];
  constexpr int D = P == 4 ? 8 : 16;      // frames of weights in flight
  constexpr int ES = BF16 ? 2 : 4;
  const int lane = threadIdx.x, b = blockIdx.x;
  const int U = a.U, T = a.T, K = a.K;
  const int A = FLD ? K + 1 : 1;
  const int NPL = FLD ? a.planes : 1;
  const int NW = NPL * P;                 // decision words per frame
  int nf = a.nfr[b];
  nf = nf < 0 ? 0 : (nf > T ? T : nf);

  // ---- outputs of an unaligned utterance; the backtrace overwrites its own
  long long* out = a.out + (long long)b * T * A;
  for (long long i = lane; i < (long long)T * A; i += 64) out[i] = 0;
  long long* lfr = a.frames ? a.frames + (long long)b * U : nullptr;
  if (lfr)
    for (int i = lane; i < U; i += 64) lfr[i] = -1;

  // ---- string positions: context state and label class
  int ob[P], ol[P];
  const StringLds sl = string_prologue<P, 64, 0>(a, b, lane, lane, a_sm, ob, ol);
  const int* yt = sl.yt;
  unsigned long long* dec = (unsigned long long*)sl.region;  // decisions / chunk

  // ---- forward
  const long long FR = (long long)a.C * a.R;
  const unsigned char* wbase = a.W + (long long)b * T * FR * ES;
  unsigned long long* gdec = a.dec_lds ? nullptr : a.ws + (long long)b * T * NW;
  float al[P];
#pragma unroll
  for (int j = 0; j < P; ++j) al[j] = (lane == 0 && j == 0) ? 0.f : -kInf;
  float pb[D][P], pl[D][P];
  if (nf > 0) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const unsigned char* wf = wbase + (long long)(d < nf ? d : nf - 1) * FR * ES;
#pragma unroll
      for (int j = 0; j < P; ++j) {
        pb[d][j] = ldw<BF16>(wf, ob[j]);
        pl[d][j] = ldw<BF16>(wf, ol[j]);
      }
    }
  }
  for (int t0 = 0; t0 < nf; t0 += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int t = t0 + d;
      if (t >= nf) break;
      float wb[P], wl[P];
#pragma unroll
      for (int j = 0; j < P; ++j) {
        wb[j] = pb[d][j];
        wl[j] = pl[d][j];
      }
      {
        const int tn = t + D < nf ? t + D : nf - 1;
        const unsigned char* wf = wbase + (long long)tn * FR * ES;
#pragma unroll
        for (int j = 0; j < P; ++j) {
          pb[d][j] = ldw<BF16>(wf, ob[j]);
          pl[d][j] = ldw<BF16>(wf, ol[j]);
        }
      }
      unsigned long long m[FLD ? 4 * P : P];
      if constexpr (!FLD) {
        float lo[P];
#pragma unroll
        for (int j = 0; j < P; ++j) lo[j] = al[j] + wl[j];
        const float up = wave_prev(lo[P - 1], -kInf);
#pragma unroll
        for (int j = 0; j < P; ++j) {
          const float x = al[j] + wb[j];
          const float y = j ? lo[j ? j - 1 : 0] : up;
          const bool ge = x >= y;
          // position 0 has no lexical term: a NaN blank term ends the path there
          const bool lex = !ge && !(lane == 0 && j == 0);
          al[j] = ge ? x : y;
          m[j] = __ballot(lex);
        }
      } else {
        float r[P], L[P];
        int wi[P];
#pragma unroll
        for (int j = 0; j < P; ++j) {
          r[j] = al[j] + wb[j];
          L[j] = al[j];
          wi[j] = 0;
        }
        for (int i = 1; i <= K; ++i) {
          float lo[P];
#pragma unroll
          for (int j = 0; j < P; ++j) lo[j] = L[j] + wl[j];
          const float up = wave_prev(lo[P - 1], -kInf);
#pragma unroll
          for (int j = 0; j < P; ++j) {
            // L_i[u] = L_{i-1}[u-1] + lex[u-1]; -inf below position i
            L[j] = (lane * P + j >= i) ? (j ? lo[j ? j - 1 : 0] : up) : -kInf;
            const float term = L[j] + wb[j];
            if (term > r[j]) {
              r[j] = term;
              wi[j] = i;
            }
          }
        }
#pragma unroll
        for (int j = 0; j < P; ++j) al[j] = r[j];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
#pragma unroll
          for (int j = 0; j < P; ++j) m[p * P + j] = p < NPL ? __ballot((wi[j] >> p) & 1) : 0;
        }
      }
      // lane w keeps word w of the frame
      unsigned long long mine = 0;
      if constexpr (!FLD) {
#pragma unroll
        for (int j = 0; j < P; ++j) mine = lane == j ? m[j] : mine;
      } else {
#pragma unroll
        for (int w = 0; w < 4 * P; ++w) mine = (w < NW && lane == w) ? m[w] : mine;
      }
      if (lane < NW) {
        if (a.dec_lds) dec[(long long)t * NW + lane] = mine;
        else gdec[(long long)t * NW + lane] = mine;
      }
    }
  }
  // alpha_T at num_labels
  const int nlb = a.nlab[b];
  const int fin = (nlb >= 0 && nlb <= U) ? nlb : -1;
  float fv = -kInf;
  if (fin >= 0) {
    float mine = al[0];
#pragma unroll
    for (int j = 1; j < P; ++j) mine = (fin % P) == j ? al[j] : mine;
    fv = __shfl(mine, fin / P, 64);
  }
  if (lane == 0) a.dist[b] = fv;
  __syncthreads();  // the rows' fill and the decisions, before lane 0's stores / loads
  if (!(fv > -kInf)) return;  // unaligned (wave-uniform)

  // ---- backtrace: chunks of whole frames, the last first
  int q = fin;
  const int F = a.dec_lds ? (nf > 0 ? nf : 1) : a.chunk;
  for (int t1 = nf; t1 > 0; t1 -= F) {
    const int t0 = t1 - F > 0 ? t1 - F : 0;
    if (!a.dec_lds) {
      const unsigned long long* src = gdec + (long long)t0 * NW;
      for (int i = lane; i < (t1 - t0) * NW; i += 64) dec[i] = src[i];
      __syncthreads();
    }
    if (lane == 0) {
      if constexpr (!FLD) {
#pragma unroll 4
        for (int t = t1 - 1; t >= t0; --t) {
          // the whole row: its address does not depend on q
          const unsigned long long* row = dec + (long long)(t - t0) * P;
          unsigned long long w = row[0];
#pragma unroll
          for (int j = 1; j < P; ++j) w = (q % P) == j ? row[j] : w;
          const int d = q > 0 ? (int)((w >> (q / P)) & 1) : 0;
          if (d) {
            --q;
            out[t] = yt[q];
            if (lfr) lfr[q] = t;
          }
        }
      } else {
        for (int t = t1 - 1; t >= t0; --t) {
          const unsigned long long* row = dec + (long long)(t - t0) * NW;
          int wi = 0;
          for (int p = 0; p < NPL; ++p) wi |= (int)((row[p * P + q % P] >> (q / P)) & 1) << p;
          wi = wi > q ? q : (wi > K ? K : wi);  // never true for finite weights
          for (int i = 0; i < wi; ++i) {
            out[(long long)t * A + i] = yt[q - wi + i];
            if (lfr) lfr[q - wi + i] = t;
          }
          q -= wi;
        }
      }
    }
    if (!a.dec_lds) __syncthreads();
  }
}

struct AlignPlan : StringPlan {
  int planes, NW, chunk;
};

// Validates the shape and lays out LDS / workspace.
int align_plan(const lt_graph* g, const lt_table_problem* pb, AlignPlan* pl) {
  if (int rc = table_check("lt_table_align", g, pb, kChkString, [&] {
        if (pb->max_labels > 255) return fail(LT_EUNSUPPORTED, "lt_table_align: max_labels > 255");
        if (g->expansions > 15) return fail(LT_EUNSUPPORTED, "lt_table_align: expansions > 15");
        return LT_OK;
      }))
    return rc;
  pl->P = string_positions(pb->max_labels);
  pl->planes = 1;
  while ((1 << pl->planes) < g->expansions + 1) ++pl->planes;
  pl->NW = pl->planes * pl->P;
  pl->chunk = std::max(1, kAlignChunk / (8 * pl->NW));
  // ctx, yn, yt; a frame of decisions is NW words
  string_layout(g, pb, 3LL * 4 * 64 * pl->P, 8LL * pl->NW, 8LL * pl->NW * pl->chunk, pl);
  return LT_OK;
}

}  // namespace

extern "C" {

int lt_table_align_workspace_bytes(const lt_graph* g, const lt_table_problem* pb, size_t* bytes) {
  AlignPlan pl;
  if (int rc = align_plan(g, pb, &pl)) return rc;
  if (bytes) *bytes = pl.ws;
  return LT_OK;
}

int lt_table_align(const lt_graph* g, const lt_table_problem* pb, const void* W,
                   const int32_t* num_frames, const int32_t* labels, const int32_t* num_labels,
                   int64_t* alignment_labels, int64_t* label_frames, float* path_weight,
                   void* workspace, size_t workspace_bytes, void* stream) {
  AlignPlan pl;
  if (int rc = align_plan(g, pb, &pl)) return rc;
  if (pb->batch == 0) return LT_OK;
  if ((!W && pb->max_frames > 0) || !num_frames || !num_labels || !path_weight ||
      (!alignment_labels && pb->max_frames > 0) || (pb->max_labels > 0 && !labels))
    return fail(LT_EINVAL, "null pointer");
  const bool bf16 = pb->weight_dtype == LT_DTYPE_BF16;
  if (((uintptr_t)W & (bf16 ? 1 : 3)) || ((uintptr_t)num_frames & 3) || ((uintptr_t)labels & 3) ||
      ((uintptr_t)num_labels & 3) || ((uintptr_t)alignment_labels & 7) ||
      ((uintptr_t)label_frames & 7) || ((uintptr_t)path_weight & 3) || ((uintptr_t)workspace & 7))
    return fail(LT_EINVAL, "misaligned pointer");
  if (pl.ws && (!workspace || workspace_bytes < pl.ws))
    return fail(LT_EINVAL, "workspace too small");
  AArgs a;
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
  a.K = g->expansions;
  a.planes = pl.planes;
  a.dec_lds = pl.hist_lds;
  a.stage_tab = pl.stage_tab;
  a.chunk = pl.chunk;
  hipStream_t st = (hipStream_t)stream;
  return dispatch(bf16, pl.P, [&](auto bf, auto p) {
    constexpr bool BF16 = decltype(bf)::value;
    constexpr int P = decltype(p)::value;
    auto k = a.K > 0 ? align_kernel<BF16, P, true> : align_kernel<BF16, P, false>;
    return launch(k, dim3(a.B), dim3(64), pl.lds, st, a, "alignment");
  });
}

}  // extern "C"
