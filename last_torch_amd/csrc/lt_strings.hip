// lt_strings.hip -- the weights of N label strings per utterance on the
// utterance's one W, and the dense gradient of a linear combination of them
// (include/lt_strings.h has the definition): what consumes an N-best list.
//
// strings_fwd_kernel   grid (utterance, group of 8 hypotheses, direction),
//   512 threads. One wave is one hypothesis; the 8 waves of a workgroup read
//   the same frames of W.
//   prologue   every wave loads its labels, its lane 0 walks the context
//              states (the table staged in LDS while it is small), every lane
//              keeps the two weight offsets of its P = ceil((U+1)/64)
//              consecutive positions in registers
//   ring       the workgroup stages whole frames one slice of L frames ahead
//              into a two-slice LDS ring: 16-byte loads issued before a slice
//              is consumed, written to the other half after it, one barrier a
//              slice (lt_beam.hip's scheme) -- upwards from frame 0 for
//              direction 0, downwards from frame nf-1 for direction 1. A frame
//              is fetched once per 8 hypotheses.
//   no ring    a frame larger than a slice (32 KiB) is read from memory by
//              each wave, row by row
//   frame      two LDS reads a position, the neighbour's value by a DPP wave
//              shift, one log-add-exp; the vector is kept relative to an
//              integer offset, floor of its wave max
//   history    (want_history) before each frame the wave stores its row and
//              the row's offset: direction 0 alpha_t, direction 1 beta_{t+1}
// strings_bwd_kernel   grid (utterance, block of kFB frames), 512 threads, no
//   recursion. Per frame: zero a 64-bit integer image of the frame in LDS;
//   every thread takes (hypothesis, position) pairs in turn, forms the blank
//   and the lexical term grad_n * exp((offsets) + (fractions)), converts them
//   to fixed point and adds them to their cells (ds_add_u64); behind a barrier
//   the image is converted to fp32 and stored with 16-byte nontemporal stores,
//   zeros included. Integer adds commute: no order, no float atomics.
#include "lt_string_common.h"

namespace {

constexpr int kStrThreads = 512;
constexpr int kStrWaves = kStrThreads / 64;  // hypotheses of a workgroup
constexpr int kStrKpt = 4;                   // 16-byte loads a thread holds per slice
constexpr int kStrMaxN = 64;
constexpr int kFB = 4;              // frames of a backward workgroup (at least)
constexpr int kBwdFixed = 1280;     // LDS of the backward beside the image

struct SArgs {
  const unsigned char* W;
  const int* nfr;
  const int* table;   // [C, V]
  const int* labels;  // [B, N, U]
  const int* nlab;    // [B, N]
  float* score;       // [B, N]
  float* hist;        // [2, B*N, T, SP] row values relative to the row's offset
  float* hoff;        // [2, B*N, T] row offsets
  int* cells;         // [B*N, 2, SP]: ctx_u * R, label class
  float2* spair;      // [B*N] score as (offset, fraction); (-inf, 0): none
  int B, T, U, C, V, R, N;
  int L, capW, stage_tab, want_hist;
};

// The ring's slice i of an utterance, a byte range widened to whole 16-byte
// granules: frames [i*L, min(nf, (i+1)*L)) going up, [max(0, nf-(i+1)*L),
// nf-i*L) going down.
struct StrSlice {
  unsigned long long gw;  // 16-byte aligned start
  int nW, ta, tb, mis;    // granules, frames [ta, tb), bytes before frame ta
};
LT_DEVINL StrSlice str_slice(const unsigned char* w, long long fw, int nf, int L, bool rev, int i) {
  StrSlice r;
  if (!rev) {
    r.ta = i * L;
    r.tb = r.ta + L < nf ? r.ta + L : nf;
  } else {
    r.tb = nf - i * L;
    r.ta = r.tb - L > 0 ? r.tb - L : 0;
  }
  const unsigned long long gw = (unsigned long long)(w + (long long)r.ta * fw);
  r.mis = (int)(gw & 15);
  r.nW = (int)((r.mis + (unsigned long long)(r.tb - r.ta) * fw + 15) >> 4);
  r.gw = gw & ~15ull;
  return r;
}
// granule j (granules past the slice repeat its first one: in range, never stored)
LT_DEVINL uint4 str_granule(const StrSlice& r, int j) {
  return *(const uint4*)(j < r.nW ? r.gw + 16ull * j : r.gw);
}

template <int P>
LT_DEVINL void store_row(float* row, int lane, const float (&v)[P]) {
  if constexpr (P == 1) row[lane] = v[0];
  else if constexpr (P == 2) ((float2*)row)[lane] = make_float2(v[0], v[1]);
  else ((float4*)row)[lane] = make_float4(v[0], v[1], v[2], v[3]);
}

// One frame of one hypothesis: wf the frame's W [C, R] (LDS or memory).
template <bool BF16, int P, bool REV>
LT_DEVINL void str_step(const unsigned char* wf, const int (&ob)[P], const int (&ol)[P],
                        float (&v)[P], float& off, int U, int lane) {
  float wb[P], wl[P], nv[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    wb[j] = ldw<BF16>(wf, ob[j]);
    wl[j] = ldw<BF16>(wf, ol[j]);
  }
  if constexpr (!REV) {
    float lv[P];  // the arc leaving u: alpha_t[u] + lex_t[u]
#pragma unroll
    for (int j = 0; j < P; ++j) lv[j] = v[j] + wl[j];
    const float pv = wave_prev(lv[P - 1], -kInf);
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const float lo = j ? lv[j ? j - 1 : 0] : pv;
      nv[j] = lane * P + j > U ? -kInf : t_lae(v[j] + wb[j], lo);
    }
  } else {
    const float nx = wave_next(v[0], -kInf);
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const int u = lane * P + j;
      const float r = j == P - 1 ? nx : v[j == P - 1 ? j : j + 1];
      const float to = u < U ? wl[j] + r : -kInf;  // no arc leaves position U
      nv[j] = u > U ? -kInf : t_lae(wb[j] + v[j], to);
    }
  }
  float mx = nv[0];
#pragma unroll
  for (int j = 1; j < P; ++j) mx = fmaxf(mx, nv[j]);
  mx = wave_max(mx);
  const float fl = __builtin_isfinite(mx) ? floorf(mx) : 0.f;
  off += fl;
#pragma unroll
  for (int j = 0; j < P; ++j) v[j] = nv[j] - fl;
}

template <bool BF16, int P, bool RING>
__global__ __launch_bounds__(kStrThreads) void strings_fwd_kernel(const SArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char st_sm[];
  constexpr int SP = 64 * P;
  constexpr int ES = BF16 ? 2 : 4;
  constexpr int NT = kStrThreads;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x, n = blockIdx.y * kStrWaves + wave;
  const bool rev = blockIdx.z == 1;
  const bool live = n < a.N;  // wave-uniform; a dead wave only stages
  const int U = a.U, T = a.T;
  int nf = a.nfr[b];
  nf = nf < 0 ? 0 : (nf > T ? T : nf);
  const long long bn = (long long)b * a.N + n, BN = (long long)a.B * a.N;

  // ---- prologue: per wave ob [SP], yn [SP]; behind them the table, then the ring
  int* wob = (int*)st_sm + wave * 2 * SP;
  int* wyn = wob + SP;
  unsigned char* region = st_sm + kStrWaves * 2 * SP * 4;
  int* tab = (int*)region;
  if (live)
    for (int u = lane; u < SP; u += 64) {
      int y = u < U ? a.labels[bn * U + u] : 0;
      if (y < 0 || y > a.V) y = 0;
      wyn[u] = y;
    }
  if (a.stage_tab)
    for (int i = tid; i < a.C * a.V; i += NT) tab[i] = a.table[i];
  __syncthreads();
  if (live && lane == 0) {
    // positions past U repeat U's state with label class 1: loads in range
    const int* tb = a.stage_tab ? tab : a.table;
    int c = 0;
    for (int u = 0; u < SP; ++u) {
      const int y = wyn[u];
      wob[u] = c * a.R;
      wyn[u] = y < 1 ? 1 : y;
      if (y != 0) c = tb[c * a.V + y - 1];
    }
  }
  __syncthreads();
  int ob[P], ol[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    ob[j] = live ? wob[lane * P + j] : 0;
    ol[j] = ob[j] + (live ? wyn[lane * P + j] : 0);
  }
  if (a.want_hist && live && !rev)
    for (int u = lane; u < SP; u += 64) {
      a.cells[bn * 2 * SP + u] = wob[u];
      a.cells[bn * 2 * SP + SP + u] = wyn[u];
    }
  __syncthreads();  // the table's image is dead: the ring may overwrite it

  const int nlb = live ? a.nlab[bn] : -1;
  const int fin = (nlb >= 0 && nlb <= U) ? nlb : -1;
  float v[P], off = 0.f;
#pragma unroll
  for (int j = 0; j < P; ++j) v[j] = (rev ? lane * P + j == fin : lane * P + j == 0) ? 0.f : -kInf;

  const long long FWb = (long long)a.C * a.R * ES;
  const unsigned char* wutt = a.W + (long long)b * T * FWb;
  float* hrow = a.hist + ((rev ? BN : 0) + bn) * T * SP;
  float* horow = a.hoff + ((rev ? BN : 0) + bn) * T;

  // frame t of this wave: the row before it, then the step
  auto frame = [&](const unsigned char* wf, int t) {
    if (a.want_hist) {
      store_row<P>(hrow + (long long)t * SP, lane, v);
      if (lane == 0) horow[t] = off;
    }
    if (!rev) str_step<BF16, P, false>(wf, ob, ol, v, off, U, lane);
    else str_step<BF16, P, true>(wf, ob, ol, v, off, U, lane);
  };

  if constexpr (RING) {
    const int sliceB = 16 * a.capW;
    const int nsl = (nf + a.L - 1) / a.L;
    uint4 rg[kStrKpt] = {};
    auto load = [&](int i) {
      const StrSlice r = str_slice(wutt, FWb, nf, a.L, rev, i);
#pragma unroll
      for (int k = 0; k < kStrKpt; ++k) rg[k] = str_granule(r, tid + k * NT);
    };
    auto store = [&](int i) {
      const StrSlice r = str_slice(wutt, FWb, nf, a.L, rev, i);
      unsigned char* buf = region + (i & 1) * sliceB;
#pragma unroll
      for (int k = 0; k < kStrKpt; ++k)
        if (tid + k * NT < r.nW) *(uint4*)(buf + 16 * (tid + k * NT)) = rg[k];
    };
    if (nsl > 0) {
      load(0);
      store(0);
    }
    __syncthreads();
    for (int i = 0; i < nsl; ++i) {
      if (i + 1 < nsl) load(i + 1);
      if (live) {
        const StrSlice r = str_slice(wutt, FWb, nf, a.L, rev, i);
        const unsigned char* wsl = region + (i & 1) * sliceB + r.mis;
        for (int k = 0; k < r.tb - r.ta; ++k) {
          const int t = rev ? r.tb - 1 - k : r.ta + k;
          frame(wsl + (long long)(t - r.ta) * FWb, t);
        }
      }
      if (i + 1 < nsl) store(i + 1);
      __syncthreads();
    }
  } else {
    if (live)
      for (int k = 0; k < nf; ++k) {
        const int t = rev ? nf - 1 - k : k;
        frame(wutt + (long long)t * FWb, t);
      }
  }

  // ---- direction 0: alpha_nf[nl]
  if (rev || !live) return;
  if (fin < 0) {
    if (lane == 0) {
      a.score[bn] = -kInf;
      if (a.want_hist) a.spair[bn] = make_float2(-kInf, 0.f);
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < P; ++j)
    if (lane * P + j == fin) {
      const bool ok = __builtin_isfinite(v[j]) && __builtin_isfinite(off);
      a.score[bn] = ok ? off + v[j] : -kInf;
      if (a.want_hist) a.spair[bn] = ok ? make_float2(off, v[j]) : make_float2(-kInf, 0.f);
    }
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------
struct SBArgs {
  const unsigned char* W;
  const int* nfr;
  const int* nlab;
  const float* score;
  const float* grad;
  float* dW;
  const float* hist;
  const float* hoff;
  const int* cells;
  const float2* spair;
  int B, T, U, C, V, R, N, SP, FB;
};

typedef float v4f __attribute__((ext_vector_type(4)));

template <bool BF16>
__global__ __launch_bounds__(kStrThreads) void strings_bwd_kernel(const SBArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sb_sm[];
  constexpr int ES = BF16 ? 2 : 4;
  constexpr int NT = kStrThreads;
  const int tid = threadIdx.x, b = blockIdx.x;
  const int T = a.T, N = a.N, SP = a.SP, U = a.U;
  const int CR = a.C * a.R;
  unsigned long long* acc = (unsigned long long*)sb_sm;  // [CR] the frame's image
  float* gs = (float*)(sb_sm + 8LL * CR);                // [64] grad of a live hypothesis, else 0
  float2* sp = (float2*)(gs + 64);                       // [64] its score (offset, fraction)
  int* nls = (int*)(sp + 64);                            // [64] its num_labels, -1: contributes nothing
  double* scl = (double*)(nls + 64);                     // scale, 1 / scale
  int* badf = (int*)(scl + 2);                           // a non-finite grad
  int nf = a.nfr[b];
  nf = nf < 0 ? 0 : (nf > T ? T : nf);
  const long long BN = (long long)a.B * N;

  // ---- the hypotheses' scalars and the utterance's fixed-point scale
  if (tid < 64) {
    const int n = tid;
    const long long bn = (long long)b * N + n;
    const float g = n < N ? a.grad[bn] : 0.f;
    const float2 s = n < N ? a.spair[bn] : make_float2(-kInf, 0.f);
    const int nl = n < N ? a.nlab[bn] : -1;
    const bool use = n < N && __builtin_isfinite(s.x) && __builtin_isfinite(a.score[bn]) &&
                     g != 0.f && __builtin_isfinite(g) && nl >= 0 && nl <= U;
    gs[n] = use ? g : 0.f;
    sp[n] = s;
    nls[n] = use ? nl : -1;
    const float gmax = wave_max(use ? fabsf(g) : 0.f);
    const unsigned long long bad = __ballot(!__builtin_isfinite(g));
    if (tid == 0) {
      // 2 N (U+1) terms of magnitude < 2^e: below 2^(c + e); the scale 2^(62 - c - e)
      int e = 0;
      if (gmax > 0.f) (void)frexpf(gmax, &e);
      const unsigned terms = 2u * (unsigned)N * (unsigned)(U + 1);
      const int c = 32 - __builtin_clz(terms - 1);
      const int k = 62 - c - e;
      scl[0] = ldexp(1.0, k);
      scl[1] = ldexp(1.0, -k);
      *badf = bad != 0;
    }
  }
  __syncthreads();
  const double scale = scl[0], inv = scl[1];
  const bool bad = *badf != 0;
  const int lsp = SP == 64 ? 6 : (SP == 128 ? 7 : 8);
  const long long FWb = (long long)CR * ES;

  for (int f = 0; f < a.FB; ++f) {
    const int t = blockIdx.y * a.FB + f;
    if (t >= T) break;
    for (int i = tid; i < CR; i += NT) acc[i] = 0ull;
    __syncthreads();
    if (t < nf && !bad) {
      const unsigned char* wf = a.W + ((long long)b * T + t) * FWb;
      for (int idx = tid; idx < N * SP; idx += NT) {
        const int n = idx >> lsp, u = idx & (SP - 1);
        const int nl = nls[n];
        if (u > nl) continue;
        const long long bn = (long long)b * N + n;
        const long long ra = bn * T + t, rb = (BN + bn) * T + t;
        const float2 s = sp[n];
        const float g = gs[n];
        // the integer offsets first, then the fractions
        const float io = (a.hoff[ra] + a.hoff[rb]) - s.x;
        const float al = a.hist[ra * SP + u];
        const int cb = a.cells[bn * 2 * SP + u];
        const int yc = a.cells[bn * 2 * SP + SP + u];
        // a workspace no forward filled: stay inside the frame
        if ((unsigned)cb >= (unsigned)CR || (unsigned)(cb + yc) >= (unsigned)CR) continue;
        const float xb = io + ((al + ldw<BF16>(wf, cb) + a.hist[rb * SP + u]) - s.y);
        const float pb = g * lt_exp(xb);
        if (pb != 0.f) atomicAdd(acc + cb, (unsigned long long)__double2ll_rn((double)pb * scale));
        if (u < nl) {
          const int cl = cb + yc;
          const float xl = io + ((al + ldw<BF16>(wf, cl) + a.hist[rb * SP + u + 1]) - s.y);
          const float pl = g * lt_exp(xl);
          if (pl != 0.f) atomicAdd(acc + cl, (unsigned long long)__double2ll_rn((double)pl * scale));
        }
      }
    }
    __syncthreads();
    // ---- the frame, zeros included: single stores up to 16-byte alignment,
    // 16-byte nontemporal stores, the tail
    const bool nan = bad && t < nf;
    auto val = [&](int i) {
      return nan ? __builtin_nanf("") : (float)((double)(long long)acc[i] * inv);
    };
    float* z = a.dW + ((long long)b * T + t) * CR;
    const int peel = (int)(((16 - ((uintptr_t)z & 15)) & 15) / 4);
    const int hd = peel < CR ? peel : CR;
    if (tid < hd) z[tid] = val(tid);
    const int n4 = (CR - hd) / 4;
    for (int i = tid; i < n4; i += NT) {
      const int e = hd + 4 * i;
      const v4f q = {val(e), val(e + 1), val(e + 2), val(e + 3)};
      __builtin_nontemporal_store(q, (v4f*)(z + e));
    }
    const int done = hd + 4 * n4;
    if (done + tid < CR) z[done + tid] = val(done + tid);
    __syncthreads();  // the image is read: the next frame may zero it
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct StrPlan {
  int P, L, capW, stage_tab, lds;
  size_t o_hoff, o_cells, o_spair, ws;
};

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// Validates the shape and lays out the forward's LDS and the workspace.
int str_plan(const char* entry, const lt_graph* g, const lt_table_problem* pb, int num_hyps,
             StrPlan* pl) {
  const std::string e(entry);
  if (int rc = table_check(entry, g, pb, kChkString, [&] {
        if (num_hyps < 1) return fail(LT_EINVAL, e + ": num_hyps < 1");
        if (g->expansions > 0)
          return fail(LT_EUNSUPPORTED, e + ": FrameLabelDependent (expansions >= 1)");
        if (pb->max_labels > 255) return fail(LT_EUNSUPPORTED, e + ": max_labels > 255");
        if (num_hyps > kStrMaxN) return fail(LT_EUNSUPPORTED, e + ": num_hyps > 64");
        return LT_OK;
      }))
    return rc;
  pl->P = string_positions(pb->max_labels);
  const long long SP = 64LL * pl->P;
  // the ring: the most whole frames whose image, with up to 15 bytes of
  // misalignment in front, is kStrKpt 16-byte loads a thread
  const long long es = pb->weight_dtype == LT_DTYPE_BF16 ? 2 : 4;
  const long long fw = (long long)g->num_states * (g->vocab_size + 1) * es;
  const long long budget = (long long)kStrThreads * kStrKpt;
  auto chunks = [](long long bytes) { return ((bytes + 15) >> 4) + 1; };
  long long L = 0;
  while (L < pb->max_frames && L < 64 && chunks((L + 1) * fw) <= budget) ++L;
  pl->L = (int)L;
  pl->capW = L ? (int)chunks(L * fw) : 0;
  const long long tabb = stage_table(g);
  pl->stage_tab = tabb ? 1 : 0;
  const long long region = std::max<long long>(2LL * 16 * pl->capW, tabb);
  pl->lds = (int)(kStrWaves * 2 * SP * 4 + ((region + 15) & ~15LL));
  const size_t BN = (size_t)pb->batch * (size_t)num_hyps, T = (size_t)pb->max_frames;
  pl->o_hoff = up256(2 * 4 * BN * T * (size_t)SP);
  pl->o_cells = pl->o_hoff + up256(2 * 4 * BN * T);
  pl->o_spair = pl->o_cells + up256(8 * BN * (size_t)SP);
  pl->ws = pl->o_spair + up256(8 * BN);
  return LT_OK;
}

}  // namespace

extern "C" {

int lt_table_strings_workspace_bytes(const lt_graph* g, const lt_table_problem* pb,
                                     int32_t num_hyps, size_t* bytes) {
  StrPlan pl;
  if (int rc = str_plan("lt_table_strings_forward", g, pb, num_hyps, &pl)) return rc;
  if (bytes) *bytes = pl.ws;
  return LT_OK;
}

int lt_table_strings_forward(const lt_graph* g, const lt_table_problem* pb, const void* W,
                             const int32_t* num_frames, int32_t num_hyps, const int32_t* labels,
                             const int32_t* num_labels, float* score, void* workspace,
                             size_t workspace_bytes, int32_t want_history, void* stream) {
  StrPlan pl;
  if (int rc = str_plan("lt_table_strings_forward", g, pb, num_hyps, &pl)) return rc;
  if (pb->batch == 0) return LT_OK;
  if ((!W && pb->max_frames > 0) || !num_frames || !num_labels || !score ||
      (pb->max_labels > 0 && !labels))
    return fail(LT_EINVAL, "null pointer");
  if (((uintptr_t)W & 15) || ((uintptr_t)num_frames & 3) || ((uintptr_t)labels & 3) ||
      ((uintptr_t)num_labels & 3) || ((uintptr_t)score & 3) || ((uintptr_t)workspace & 15))
    return fail(LT_EINVAL, "misaligned pointer");
  if (want_history && (!workspace || workspace_bytes < pl.ws))
    return fail(LT_EINVAL, "workspace too small");
  SArgs a;
  memset(&a, 0, sizeof(a));
  a.W = (const unsigned char*)W;
  a.nfr = num_frames;
  a.table = g->next_state;
  a.labels = labels;
  a.nlab = num_labels;
  a.score = score;
  if (want_history) {
    unsigned char* ws = (unsigned char*)workspace;
    a.hist = (float*)ws;
    a.hoff = (float*)(ws + pl.o_hoff);
    a.cells = (int*)(ws + pl.o_cells);
    a.spair = (float2*)(ws + pl.o_spair);
  }
  a.B = pb->batch;
  a.T = pb->max_frames;
  a.U = pb->max_labels;
  a.C = g->num_states;
  a.V = g->vocab_size;
  a.R = g->vocab_size + 1;
  a.N = num_hyps;
  a.L = pl.L;
  a.capW = pl.capW;
  a.stage_tab = pl.stage_tab;
  a.want_hist = want_history ? 1 : 0;
  const dim3 grid((unsigned)a.B, (unsigned)((a.N + kStrWaves - 1) / kStrWaves),
                  want_history ? 2u : 1u);
  return dispatch(pb->weight_dtype == LT_DTYPE_BF16, pl.P, [&](auto bf, auto p) {
    constexpr bool BF16 = decltype(bf)::value;
    constexpr int P = decltype(p)::value;
    auto k = a.L ? strings_fwd_kernel<BF16, P, true> : strings_fwd_kernel<BF16, P, false>;
    return launch(k, grid, dim3(kStrThreads), pl.lds, (hipStream_t)stream, a, "string weights");
  });
}

int lt_table_strings_backward(const lt_graph* g, const lt_table_problem* pb, const void* W,
                              const int32_t* num_frames, int32_t num_hyps, const int32_t* labels,
                              const int32_t* num_labels, const float* score, const float* grad,
                              float* dW, void* workspace, size_t workspace_bytes, void* stream) {
  (void)labels;  // the forward left the cells they name in the workspace
  StrPlan pl;
  if (int rc = str_plan("lt_table_strings_backward", g, pb, num_hyps, &pl)) return rc;
  const long long CR = (long long)g->num_states * (g->vocab_size + 1);
  const long long lds = 8 * CR + kBwdFixed;
  if (lds > kTabLds)
    return fail(LT_EUNSUPPORTED,
                "lt_table_strings_backward: 8 C (V+1) bytes of LDS accumulator past 160 KiB");
  if (pb->batch == 0 || pb->max_frames == 0) return LT_OK;
  if (!W || !num_frames || !num_labels || !score || !grad || !dW || !workspace)
    return fail(LT_EINVAL, "null pointer");
  if (((uintptr_t)W & 3) || ((uintptr_t)num_frames & 3) || ((uintptr_t)num_labels & 3) ||
      ((uintptr_t)score & 3) || ((uintptr_t)grad & 3) || ((uintptr_t)dW & 3) ||
      ((uintptr_t)workspace & 15))
    return fail(LT_EINVAL, "misaligned pointer");
  if (workspace_bytes < pl.ws) return fail(LT_EINVAL, "workspace too small");
  SBArgs a;
  memset(&a, 0, sizeof(a));
  const unsigned char* ws = (const unsigned char*)workspace;
  a.W = (const unsigned char*)W;
  a.nfr = num_frames;
  a.nlab = num_labels;
  a.score = score;
  a.grad = grad;
  a.dW = dW;
  a.hist = (const float*)ws;
  a.hoff = (const float*)(ws + pl.o_hoff);
  a.cells = (const int*)(ws + pl.o_cells);
  a.spair = (const float2*)(ws + pl.o_spair);
  a.B = pb->batch;
  a.T = pb->max_frames;
  a.U = pb->max_labels;
  a.C = g->num_states;
  a.V = g->vocab_size;
  a.R = g->vocab_size + 1;
  a.N = num_hyps;
  a.SP = 64 * pl.P;
  a.FB = std::max(kFB, (a.T + 65534) / 65535);
  const dim3 grid((unsigned)a.B, (unsigned)((a.T + a.FB - 1) / a.FB));
  return dispatch(pb->weight_dtype == LT_DTYPE_BF16, [&](auto bf) {
    constexpr bool BF16 = decltype(bf)::value;
    return launch(strings_bwd_kernel<BF16>, grid, dim3(kStrThreads), (int)lds,
                  (hipStream_t)stream, a, "string weights backward");
  });
}

}  // extern "C"
