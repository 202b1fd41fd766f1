// lt_paths.hip -- the weight of given alignment paths (lt_table_path_score)
// and the scatter of one scalar per path onto the arcs it takes
// (lt_table_path_scatter), for any next-state table x FrameDependent. The
// operations are defined in include/lt_paths.h.
//
// path_score    one wave per (utterance, path); the waves of a workgroup
//               belong to one utterance and share the table staged in LDS.
//   walk        the state before a frame depends on every label before it,
//               but only non-blank labels move it: 64 labels are loaded
//               coalesced, the non-blank lanes balloted, and the wave steps
//               over the set bits alone -- one dependent table read each
//               (LDS, or memory when the table is past kPathTab), the state
//               wave-uniform. Lane t % 64 keeps the state before frame t.
//   gather      every lane reads its own frame's W[b,t,q_t,y_t] and puts it
//               into the path's LDS row; states go out as coalesced stores.
//   sum         fp32 adds from the last live frame to the first over the LDS
//               row (the order of lt_sample.hip, so sampled labels score to
//               the sampler's weight bit for bit).
// path_scatter  one kernel, the zeros included (a workgroup zeroes the rows it
//               owns, as lt_table_string_scatter does); one thread owns a
//               (b, t) column of dW and adds the paths in ascending s, so arcs
//               that paths share are summed in a fixed order without atomics.
#include "lt_string_common.h"

namespace {

struct PArgs {
  const unsigned char* W;
  const int* nfr;
  const long long* labels;  // [B, S, T]
  const int* table;         // [C, V] next state of (p, y)
  float* pw;                // [B, S]
  int* states;              // [B, S, T] or null
  int B, T, C, V, R, S;
  int wpb;        // waves (paths) per workgroup
  int nblk;       // workgroups per utterance
  int Tp;         // floats of a path's LDS row: T rounded up to 64
  int stage_tab;  // the table is staged in LDS
};

constexpr int kPathTab = 64 * 1024;   // largest table staged in LDS

template <bool BF16>
__global__ __launch_bounds__(512) void path_score_kernel(const PArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char p_sm[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x / a.nblk;
  const int s = (blockIdx.x % a.nblk) * a.wpb + wave;
  const int T = a.T, C = a.C, V = a.V, R = a.R;
  int* tab_s = (int*)p_sm;
  const int tabn = a.stage_tab ? C * V : 0;
  if (a.stage_tab) {
    for (int i = tid; i < tabn; i += blockDim.x) tab_s[i] = a.table[i];
    __syncthreads();
  }
  if (s >= a.S) return;  // wave-uniform, after the only barrier
  const int* tab = a.stage_tab ? tab_s : a.table;
  float* wrow = (float*)(p_sm + 4 * (long long)tabn) + (long long)wave * a.Tp;
  int nf = a.nfr[b];
  nf = nf < 0 ? 0 : (nf > T ? T : nf);
  const long long row = ((long long)b * a.S + s) * T;
  const long long* lab = a.labels + row;
  int* st = a.states ? a.states + row : nullptr;
  const long long FW = (long long)C * R;  // weights of a frame
  const long long wutt = (long long)b * T * FW;

  int q = 0;
  bool valid = true;
  for (int base = 0; base < nf; base += 64) {
    const int t = base + lane;
    const bool live = t < nf;
    const long long y64 = live ? lab[t] : 0;
    if (__ballot(y64 < 0 || y64 > V)) {
      valid = false;
      break;
    }
    const int y = (int)y64;
    int myq = q;  // the state before this lane's frame
    for (unsigned long long m = __ballot(y > 0); m; m &= m - 1) {
      const int l = __ffsll((long long)m) - 1;
      const int yl = __builtin_amdgcn_readlane(y, l);
      q = __builtin_amdgcn_readfirstlane(tab[q * V + yl - 1]);
      if (lane > l) myq = q;
    }
    wrow[t] = live ? ldw<BF16>(a.W, wutt + (long long)t * FW + (long long)myq * R + y) : 0.f;
    if (st && t < T) st[t] = live ? myq : -1;
  }
  if (st) {
    // padding frames past the last label chunk; the whole row of an invalid path
    const int from = valid ? ((nf + 63) & ~63) : 0;
    for (int i = from + lane; i < T; i += 64) st[i] = -1;
  }
  float wsum = -kInf;
  if (valid) {
    // the row was written by other lanes of this wave
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    wsum = 0.f;
    int t = nf - 1;
    for (; t >= 3; t -= 4) {
      const float w0 = wrow[t], w1 = wrow[t - 1], w2 = wrow[t - 2], w3 = wrow[t - 3];
      wsum += w0;
      wsum += w1;
      wsum += w2;
      wsum += w3;
    }
    for (; t >= 0; --t) wsum += wrow[t];
  }
  if (lane == 0) a.pw[(long long)b * a.S + s] = wsum;
}

struct CArgs {
  const int* nfr;
  const long long* labels;  // [B, S, T]
  const int* states;        // [B, S, T]
  const float* grad;        // [B, S]
  float* dW;                // [B, T, C, R]
  int B, T, C, V, R, S;
  int chunks;  // workgroups per utterance
};

constexpr int kScatterFrames = 64;  // frames a workgroup owns
constexpr int kScatterThreads = 256;

// A workgroup is the only writer of its rows [t0, t0 + kScatterFrames) of
// utterance b, as in lt_table_string_scatter (lt_align_expect.hip): it stores
// zeros over all of them, meets at a barrier (__syncthreads: a workgroup-scope
// release / acquire pair), and then thread t - t0 alone adds the paths'
// scalars into column (b, t), in ascending s.
__global__ __launch_bounds__(kScatterThreads) void path_scatter_kernel(const CArgs a) {
  const int tid = threadIdx.x;
  const int b = blockIdx.x / a.chunks;
  const int t0 = (blockIdx.x % a.chunks) * kScatterFrames;
  const int tz = t0 + kScatterFrames < a.T ? t0 + kScatterFrames : a.T;
  const long long FR = (long long)a.C * a.R;
  float* z = a.dW + ((long long)b * a.T + t0) * FR;
  zero_rows(z, (long long)(tz - t0) * FR, tid, kScatterThreads);
  int nf = a.nfr[b];
  nf = nf < 0 ? 0 : (nf > a.T ? a.T : nf);
  if (t0 >= nf) return;  // workgroup-uniform: padding frames stay zero
  __syncthreads();
  const int t = t0 + tid;
  if (tid >= kScatterFrames || t >= nf) return;
  float* col = z + (long long)tid * FR;
  const long long first = (long long)b * a.S * a.T + t;
  for (int s = 0; s < a.S; ++s) {
    const long long i = first + (long long)s * a.T;
    const int q = a.states[i];
    const long long y = a.labels[i];
    if (q < 0 || q >= a.C || y < 0 || y > a.V) continue;
    // this thread alone touches the column: a plain read-modify-write
    float* cell = col + (long long)q * a.R + y;
    *cell = *cell + a.grad[(long long)b * a.S + s];
  }
}

// The checks the two entry points share; the messages name the caller.
int path_check(const char* entry, const lt_graph* g, const lt_table_problem* pb, int num_paths) {
  if (int rc = table_check(entry, g, pb, 0, [&] {
        if (num_paths < 1) return fail(LT_EINVAL, "num_paths < 1");
        if (g->expansions >= 1)
          return fail(LT_EUNSUPPORTED,
                      std::string(entry) + ": FrameLabelDependent (expansions >= 1)");
        return check_arrays(g, false);
      }))
    return rc;
  if ((long long)num_paths * pb->batch > 0x7fffffffLL)
    return fail(LT_EUNSUPPORTED, std::string(entry) + ": 2^31 paths or more");
  return LT_OK;
}

struct ScorePlan {
  int wpb, nblk, Tp, stage_tab, lds;
};

// Lays out the workgroup's LDS: the table while it fits, one row of T floats
// per path, as many paths (at most 8) as fit next to it.
int score_plan(const lt_graph* g, const lt_table_problem* pb, int num_paths, ScorePlan* pl) {
  const long long rowb = 4LL * (((long long)pb->max_frames + 63) & ~63LL);
  long long tabb = stage_table(g, kPathTab);
  if (tabb + rowb > kTabLds) tabb = 0;
  if (rowb > kTabLds)
    return fail(LT_EUNSUPPORTED, "lt_table_path_score: more frames than the LDS rows hold");
  long long wpb = num_paths < 8 ? num_paths : 8;
  while (wpb > 1 && tabb + wpb * rowb > kTabLds) --wpb;
  pl->wpb = (int)wpb;
  pl->nblk = (int)((num_paths + wpb - 1) / wpb);
  if ((long long)pl->nblk * pb->batch > 0x7fffffffLL)
    return fail(LT_EUNSUPPORTED, "lt_table_path_score: 2^31 paths or more");
  pl->Tp = (int)(rowb / 4);
  pl->stage_tab = tabb ? 1 : 0;
  pl->lds = (int)(tabb + wpb * rowb);
  return LT_OK;
}

}  // namespace

extern "C" {

int lt_table_path_score(const lt_graph* g, const lt_table_problem* pb, const void* W,
                        const int32_t* num_frames, const int64_t* labels, int32_t num_paths,
                        float* path_weight, int32_t* states, void* stream) {
  if (int rc = path_check("lt_table_path_score", g, pb, num_paths)) return rc;
  ScorePlan pl;
  if (int rc = score_plan(g, pb, num_paths, &pl)) return rc;
  if (pb->batch == 0) return LT_OK;
  if (!path_weight || !num_frames || ((!W || !labels) && pb->max_frames > 0))
    return fail(LT_EINVAL, "lt_table_path_score: null pointer");
  if (((uintptr_t)W & 3) || ((uintptr_t)num_frames & 3) || ((uintptr_t)labels & 7) ||
      ((uintptr_t)path_weight & 3) || ((uintptr_t)states & 3))
    return fail(LT_EINVAL, "misaligned pointer");
  PArgs a;
  memset(&a, 0, sizeof(a));
  a.W = (const unsigned char*)W;
  a.nfr = num_frames;
  a.labels = (const long long*)labels;
  a.table = g->next_state;
  a.pw = path_weight;
  a.states = states;
  a.B = pb->batch;
  a.T = pb->max_frames;
  a.C = g->num_states;
  a.V = g->vocab_size;
  a.R = g->vocab_size + 1;
  a.S = num_paths;
  a.wpb = pl.wpb;
  a.nblk = pl.nblk;
  a.Tp = pl.Tp;
  a.stage_tab = pl.stage_tab;
  return dispatch(pb->weight_dtype == LT_DTYPE_BF16, [&](auto bf) {
    return launch(path_score_kernel<decltype(bf)::value>, dim3((unsigned)(a.B * pl.nblk)),
                  dim3(64 * pl.wpb), pl.lds, (hipStream_t)stream, a, "path score");
  });
}

int lt_table_path_scatter(const lt_graph* g, const lt_table_problem* pb,
                          const int32_t* num_frames, const int64_t* labels,
                          const int32_t* states, int32_t num_paths, const float* grad, float* dW,
                          void* stream) {
  if (int rc = path_check("lt_table_path_scatter", g, pb, num_paths)) return rc;
  if (pb->batch == 0 || pb->max_frames == 0) return LT_OK;
  if (!num_frames || !labels || !states || !grad || !dW)
    return fail(LT_EINVAL, "lt_table_path_scatter: null pointer");
  if (((uintptr_t)num_frames & 3) || ((uintptr_t)labels & 7) || ((uintptr_t)states & 3) ||
      ((uintptr_t)grad & 3) || ((uintptr_t)dW & 3))
    return fail(LT_EINVAL, "misaligned pointer");
  const int chunks = (pb->max_frames + kScatterFrames - 1) / kScatterFrames;
  if ((long long)chunks * pb->batch > 0x7fffffffLL)
    return fail(LT_EUNSUPPORTED, "lt_table_path_scatter: 2^31 workgroups or more");
  CArgs a;
  memset(&a, 0, sizeof(a));
  a.nfr = num_frames;
  a.labels = (const long long*)labels;
  a.states = states;
  a.grad = grad;
  a.dW = dW;
  a.B = pb->batch;
  a.T = pb->max_frames;
  a.C = g->num_states;
  a.V = g->vocab_size;
  a.R = g->vocab_size + 1;
  a.S = num_paths;
  a.chunks = chunks;
  return launch(path_scatter_kernel, dim3((unsigned)(chunks * a.B)), dim3(kScatterThreads), 0,
                (hipStream_t)stream, a, "path scatter");
}

}  // extern "C"
