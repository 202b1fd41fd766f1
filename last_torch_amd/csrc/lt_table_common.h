// lt_table_common.h -- the frame-serial skeleton the one-workgroup-per-
// utterance kernels over a next-state table share (lt_table.hip: the
// semiring forward / backward; lt_expect.hip: the expectation pair): the
// graph's LDS copy, the running logsumexp, the integer-shift slots, and the
// register staging of a frame's weights and of a history row.
#ifndef LT_TABLE_COMMON_H_
#define LT_TABLE_COMMON_H_

#include "lt_kernels.h"

namespace {

// Copies the graph arrays to LDS at g (ints: in_off [C+1], in_arc [C*V],
// table [C*V]) when GST, and returns the arrays to use (compile-time choice,
// so the compiler knows which memory every access goes to). A: kernel
// arguments with C, V, in_off, in_arc and table.
template <bool GST, typename A>
LT_DEVINL void t_graph(const A& a, int* g, const int** in_off, const int** in_arc,
                       const int** table) {
  if constexpr (!GST) {
    *in_off = a.in_off;
    *in_arc = a.in_arc;
    *table = a.table;
    return;
  }
  const int C = a.C, CV = a.C * a.V;
  for (int i = threadIdx.x; i <= C; i += blockDim.x) g[i] = a.in_off[i];
  for (int i = threadIdx.x; i < CV; i += blockDim.x) {
    const int id = a.in_arc[i];
    const int p = id / a.V;
    g[C + 1 + i] = p | ((id - p * a.V) << 16);  // DenGraphP packing
    g[C + 1 + CV + i] = a.table[i];
  }
  *in_off = g;
  *in_arc = g + C + 1;
  *table = g + C + 1 + CV;
}

LT_DEVINL float t_safe(float x) { return __builtin_isfinite(x) ? x : 0.f; }
// _LogAddExp (semirings.py:248-255)
LT_DEVINL float t_lae(float a, float b) {
  const float m = fmaxf(a, b);
  const float c = t_safe(m);
  return c + lt_log_acc(lt_exp(a - c) + lt_exp(b - c));
}
// running logsumexp (m, s): the result is m + log(s) with the safe max
struct Lse {
  float m = -kInf, s = 0.f;
  LT_DEVINL void add(float x) {
    if (x == -kInf) return;
    if (x > m) {
      s = s * lt_exp(m - x) + 1.f;
      m = x;
    } else {
      s += lt_exp(x - m);
    }
  }
  LT_DEVINL float get() const { return s > 0.f ? m + lt_log_acc(s) : -kInf; }
};

// Log vectors are kept relative to an integer offset near their maximum
// (exact in fp32), so a recursion over T frames rounds small numbers, not
// values of magnitude |log_z| (the tuned kernels' scheme): the
// offset after a frame is floor(max) of its new vector.
// That offset without a pass of its own: the threads that write the new
// vector's values fold them into an LDS slot (ds_max on an order-preserving
// int image) and, after the barrier that publishes the vector, every thread
// reads the slot. Three slots rotate: frame t writes slot t % 3, reads it
// after its barrier, and resets slot (t + 1) % 3 for the next frame (the
// last frame that read it was t - 2).
LT_DEVINL int t_ord(float f) {
  const int i = __float_as_int(f);
  return i >= 0 ? i : i ^ 0x7fffffff;
}
LT_DEVINL float t_unord(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff); }
struct MaxSlots {
  int* s;  // [3] in LDS
  LT_DEVINL void init() const {
    if (threadIdx.x < 3) s[threadIdx.x] = t_ord(-kInf);
  }
  LT_DEVINL void put(int t, float v) const { atomicMax(s + t % 3, t_ord(v)); }
  LT_DEVINL void reset_next(int t) const {
    if (threadIdx.x == 0) s[(t + 1) % 3] = t_ord(-kInf);
  }
  // after the barrier: the integer offset floor(max) (0 when not finite)
  LT_DEVINL float shift(int t) const {
    const float m = t_unord(s[t % 3]);
    return __builtin_isfinite(m) ? floorf(m) : 0.f;
  }
};

// Graph accessors of the context lattice (states p, in-arcs from the CSR).
struct DenGraph {
  const int* in_off;
  const int* in_arc;
  int V, R;
  LT_DEVINL int blank(int q) const { return q * R; }
  LT_DEVINL int nin(int q) const { return in_off[q + 1] - in_off[q]; }
  LT_DEVINL int pos0(int q) const { return in_off[q]; }
  LT_DEVINL void arc(int pos, int q, int* src, int* widx) const {
    (void)q;
    const int id = in_arc[pos];
    const int p = id / V;
    *src = p;
    *widx = p * R + (id - p * V) + 1;
  }
};
// The LDS copy of the CSR holds src | (label - 1) << 16 (no division).
struct DenGraphP {
  const int* in_off;
  const int* in_arc;
  int V, R;
  LT_DEVINL int blank(int q) const { return q * R; }
  LT_DEVINL int nin(int q) const { return in_off[q + 1] - in_off[q]; }
  LT_DEVINL int pos0(int q) const { return in_off[q]; }
  LT_DEVINL void arc(int pos, int q, int* src, int* widx) const {
    (void)q;
    const int v = in_arc[pos];
    const int p = v & 0xffff;
    *src = p;
    *widx = p * R + (v >> 16) + 1;
  }
};

// Register staging of a strided per-frame gather (element e -> ld(e)): the
// next frame's values are loaded while this frame computes, so a frame costs
// no memory round trip of its own (N rounds per thread; the rest is loaded
// directly when stored)
template <int N>
struct RegStage {
  float r[N];
  template <typename F>
  LT_DEVINL void fetch(int n, const F& ld) {
#pragma unroll
    for (int u = 0; u < N; ++u) {
      const int e = u * blockDim.x + threadIdx.x;
      r[u] = e < n ? ld(e) : 0.f;
    }
  }
  template <typename F>
  LT_DEVINL void store(float* dst, int n, const F& ld) const {
#pragma unroll
    for (int u = 0; u < N; ++u) {
      const int e = u * blockDim.x + threadIdx.x;
      if (e < n) dst[e] = r[u];
    }
    for (int e = N * blockDim.x + threadIdx.x; e < n; e += blockDim.x) dst[e] = ld(e);
  }
};

// Merge a running logsumexp over G aligned lanes (xor shuffles; every lane of
// the wave takes part) -- the lanes then hold the group's total.
template <int G>
LT_DEVINL void lse_merge(Lse& l) {
  for (int o = 1; o < G; o <<= 1) {
    const float m2 = __shfl_xor(l.m, o, 64), s2 = __shfl_xor(l.s, o, 64);
    const float M = fmaxf(l.m, m2);
    if (M == -kInf) {
      l.s = 0.f;
    } else {
      l.s = l.s * lt_exp(l.m - M) + s2 * lt_exp(m2 - M);
      l.m = M;
    }
  }
}

// Frame staging: the first kPf*blockDim weights of frame t+1 are loaded into
// registers while frame t is processed (one memory round trip per frame,
// hidden), the rest of a large frame in batches of kPf loads per thread.
constexpr int kPf = 8;
template <bool BF16>
struct FrameStage {
  float r[kPf];
  LT_DEVINL void fetch(const unsigned char* wf, long long FR) {
#pragma unroll
    for (int u = 0; u < kPf; ++u) {
      const long long e = (long long)u * blockDim.x + threadIdx.x;
      r[u] = (wf && e < FR) ? ldw<BF16>(wf, e) : 0.f;
    }
  }
  LT_DEVINL void store(float* wl, const unsigned char* wf, long long FR) {
#pragma unroll
    for (int u = 0; u < kPf; ++u) {
      const long long e = (long long)u * blockDim.x + threadIdx.x;
      if (e < FR) wl[e] = r[u];
    }
    for (long long e0 = (long long)kPf * blockDim.x; e0 < FR; e0 += (long long)kPf * blockDim.x) {
      float t[kPf];
#pragma unroll
      for (int u = 0; u < kPf; ++u) {
        const long long e = e0 + (long long)u * blockDim.x + threadIdx.x;
        t[u] = e < FR ? ldw<BF16>(wf, e) : 0.f;
      }
#pragma unroll
      for (int u = 0; u < kPf; ++u) {
        const long long e = e0 + (long long)u * blockDim.x + threadIdx.x;
        if (e < FR) wl[e] = t[u];
      }
    }
  }
};

// The table kernels' LDS rule (host side): a workgroup's dynamic LDS is at
// most kTabLds, and a frame is staged in LDS beside the state vectors and
// the graph only while the whole image stays within kStageBudget.
constexpr int kTabLds = 160 * 1024;
constexpr int kStageBudget = 144 * 1024;

}  // namespace

#endif  // LT_TABLE_COMMON_H_
