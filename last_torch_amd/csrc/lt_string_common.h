// lt_string_common.h -- what the feature kernels over a next-state table
// share (lt_align.hip, lt_align_post.hip, lt_align_expect.hip, lt_sample.hip,
// lt_beam.hip, lt_paths.hip, lt_expect.hip; lt_edit.hip takes fail / launch).
// Device side: the string prologue (labels, the walk of the context states,
// each lane's weight offsets), the two-wave midpoint reduce, the zero fill of
// the scatter kernels, the wave max. Host side: the refusals every entry point
// makes, the P and staged-table rules, the LDS layout of a string kernel with
// a per-frame history, the launch triple and the bf16 x P dispatch.
//
// Two kernels of lt_align_expect.hip keep code of their own that reads like
// string_prologue's:
//   align_expect_kernel  calls string_midpoint but has the prologue inline. On
//       the shared one its machine code moved by one instruction ahead of the
//       frame loops, and the all-outputs call at the bench shape measured
//       1.35 % slower than before, outside the 0.5 % spread of its batches
//       (profiles/string_common_ab.txt); with its own prologue the code is
//       the old one but for the operand order of four adds.
//   string_scatter_kernel  walks U+1 positions, not 64P, keeps no yt, and its
//       one walking thread reads the labels from memory while the other
//       threads' zero stores are in flight, so it clamps a label where it
//       reads it. A walk shared through a label functor compiled to other
//       code for it and saved six lines.
#ifndef LT_STRING_COMMON_H_
#define LT_STRING_COMMON_H_

#include <type_traits>

#include "lt_table_common.h"

namespace {

// ---------------------------------------------------------------------------
// device side
// ---------------------------------------------------------------------------

// max over the wave, wave-uniform (the whole wave must be active): four
// butterfly stages inside each DPP row, rows_fold across the rows, lane 63
// read back. (Not in lt_kernels.h: lt_pipe.hip has a wave_max of its own.)
LT_DEVINL float wave_max(float v) {
  v = dpp_max<0>(v);
  v = dpp_max<1>(v);
  v = dpp_max<2>(v);
  v = dpp_max<3>(v);
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rows_fold<true>(v)), 63));
}

// The LDS arrays of a string kernel: three int arrays of SP = 64P positions,
// MID bytes per position of the kernel's own, then the region that holds the
// staged table during the prologue and the kernel's history afterwards.
struct StringLds {
  int* ctx;  // [SP] context state of position u, times R
  int* yn;   // [SP] label class of the arc leaving u
  int* yt;   // [SP] its true label (0: epsilon)
  unsigned char* mid;
  unsigned char* region;
};

// The prologue of a workgroup of NT threads (whole waves of 64; each wave
// holds all SP positions, lane l the P consecutive ones from l*P) for
// utterance b: labels to yt, the table staged in the region while it is small
// (a.stage_tab), thread 0 walks the context states, every lane keeps the two
// weight offsets of its positions (ob: the blank arc, ol: the lexical arc),
// and a last barrier after which the table's image is dead and the region may
// be overwritten. A: kernel arguments with labels, table, U, C, V, R,
// stage_tab. lt_align.hip and lt_align_post.hip call it.
template <int P, int NT, int MID, typename A>
LT_DEVINL StringLds string_prologue(const A& a, int b, int tid, int lane, unsigned char* sm,
                                    int (&ob)[P], int (&ol)[P]) {
  constexpr int SP = 64 * P;
  StringLds s;
  s.ctx = (int*)sm;
  s.yn = s.ctx + SP;
  s.yt = s.yn + SP;
  s.mid = (unsigned char*)(s.yt + SP);
  s.region = s.mid + MID * SP;
  int* tab = (int*)s.region;
  for (int u = tid; u < SP; u += NT) {
    int y = u < a.U ? a.labels[(long long)b * a.U + u] : 0;
    if (y < 0 || y > a.V) y = 0;
    s.yt[u] = y;
  }
  if (a.stage_tab)
    for (int i = tid; i < a.C * a.V; i += NT) tab[i] = a.table[i];
  __syncthreads();
  if (tid == 0) {
    // positions past U repeat U's state with label class 1: loads in range
    auto walk = [&](const int* tb) {
      int c = 0;
      for (int u = 0; u < SP; ++u) {
        const int y = s.yt[u];
        s.ctx[u] = c * a.R;
        s.yn[u] = y < 1 ? 1 : y;
        if (y != 0) c = tb[c * a.V + y - 1];
      }
    };
    if (a.stage_tab) walk(tab);
    else walk(a.table);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < P; ++j) {
    ob[j] = s.ctx[lane * P + j];
    ol[j] = ob[j] + s.yn[lane * P + j];
  }
  __syncthreads();  // the table's image is dead: the region may be overwritten
  return s;
}

// The one meeting of the two waves of a 128-thread string kernel. Wave F
// (!rev) publishes alpha_m and wave R beta_m as (integer part, fraction) in
// mid [2, SP] (MEAN: and their conditional means mn in midm [2, SP]), ONE
// workgroup barrier, then both waves compute
//     log_prob = lpi + lpf = logsumexp_u(alpha_m[u] + beta_m[u])
// (MEAN: and E, the posterior mean of the two means' sum) from the same LDS
// words by the same instructions: bit-equal in both waves. Returns whether
// any path carries weight (wave-uniform, the same in both waves); lpi = 0,
// E = 0 when none does.
template <int P, bool MEAN>
LT_DEVINL bool string_midpoint(float2* mid, float* midm, bool rev, int lane, const float (&o)[P],
                               const float (&v)[P], const float* mn, float& lpi, float& lpf,
                               float& E) {
  constexpr int SP = 64 * P;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    mid[(rev ? SP : 0) + lane * P + j] = make_float2(o[j], v[j]);
    if constexpr (MEAN) midm[(rev ? SP : 0) + lane * P + j] = mn[j];
  }
  __syncthreads();  // history rows and the midpoint vectors
  float si[P], sf[P], sm[P];
  float mx = -kInf;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const float2 x = mid[lane * P + j], y = mid[SP + lane * P + j];
    si[j] = x.x + y.x;
    sf[j] = x.y + y.y;
    if constexpr (MEAN) sm[j] = midm[lane * P + j] + midm[SP + lane * P + j];
    mx = fmaxf(mx, si[j] + sf[j]);
  }
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) mx = fmaxf(mx, __shfl_xor(mx, s, 64));
  const bool ok = __builtin_isfinite(mx);
  lpi = ok ? floorf(mx) : 0.f;
  float sum = 0.f, ex = 0.f;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const float e = lt_exp((si[j] - lpi) + sf[j]);
    sum += e;
    if constexpr (MEAN) ex += e > 0.f ? e * sm[j] : 0.f;
  }
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    sum += __shfl_xor(sum, s, 64);
    if constexpr (MEAN) ex += __shfl_xor(ex, s, 64);
  }
  lpf = lt_log_acc(sum);
  if constexpr (MEAN) E = ok ? ex / sum : 0.f;
  return ok;
}

// Zeros over z[0, n) by a workgroup of NT threads: single stores up to
// 16-byte alignment, 16-byte stores, the tail.
LT_DEVINL void zero_rows(float* z, long long n, int tid, int NT) {
  const long long peel = (long long)(((16 - ((uintptr_t)z & 15)) & 15) / 4);
  const long long hd = peel < n ? peel : n;
  if (tid < hd) z[tid] = 0.f;
  float4* z4 = (float4*)(z + hd);
  const long long n4 = (n - hd) / 4;
  for (long long i = tid; i < n4; i += NT) z4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  const long long done = hd + 4 * n4;
  if (done + tid < n) z[done + tid] = 0.f;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
inline int fail(int code, const std::string& msg) { return lt_impl::set_error(code, msg.c_str()); }

constexpr int kStageTab = 32 * 1024;  // largest next-state table staged in LDS

// table_check flags
enum {
  kChkString = 1,     // a string entry: next_state and max_labels are checked up front
  kChkDtypeLast = 2,  // the dtype is looked at after the frame size
  kChkNoDtype = 4,    // the entry reads no weights
};

inline int check_arrays(const lt_graph* g, bool csr) {
  if (!g->next_state || (csr && (!g->in_offsets || !g->in_arcs)))
    return fail(LT_EINVAL, "null graph arrays");
  return LT_OK;
}

// The refusals every table entry point makes, in the entry's own order: the
// graph and the shape; `mid()`, the entry's own refusals (an int, LT_OK to go
// on); then "<entry>: a frame of 2^31 weights or more".
template <typename Mid>
int table_check(const char* entry, const lt_graph* g, const lt_table_problem* pb, int flags,
                const Mid& mid) {
  if (!g || !pb) return fail(LT_EINVAL, "null graph / problem");
  if (g->num_states < 1 || g->vocab_size < 1 || g->expansions < 0)
    return fail(LT_EINVAL, "bad graph (states >= 1, vocab >= 1, expansions >= 0)");
  const bool str = flags & kChkString;
  if (str)
    if (int rc = check_arrays(g, false)) return rc;
  if (pb->batch < 0 || pb->max_frames < 0 || (str && pb->max_labels < 0))
    return fail(LT_EINVAL, "negative shape");
  const bool bad_dtype = pb->weight_dtype != LT_DTYPE_F32 && pb->weight_dtype != LT_DTYPE_BF16;
  if (bad_dtype && !(flags & (kChkDtypeLast | kChkNoDtype))) return fail(LT_EINVAL, "bad dtype");
  if (int rc = mid()) return rc;
  if ((long long)g->num_states * (g->vocab_size + 1) > 0x7fffffffLL)
    return fail(LT_EUNSUPPORTED, std::string(entry) + ": a frame of 2^31 weights or more");
  if (bad_dtype && (flags & kChkDtypeLast)) return fail(LT_EINVAL, "bad dtype");
  return LT_OK;
}

// Terms (string positions) per lane of a wave that holds max_labels + 1.
inline int string_positions(int max_labels) {
  const int S = max_labels + 1;
  return S <= 64 ? 1 : (S <= 128 ? 2 : 4);
}

// Bytes of the next-state table when it is staged in LDS (at most `limit`), else 0.
inline long long stage_table(const lt_graph* g, long long limit = kStageTab) {
  const long long tabb = 4LL * g->num_states * g->vocab_size;
  return tabb <= limit ? tabb : 0;
}

// LDS and workspace of a string kernel: `fixed` bytes of prologue arrays, then
// a region that holds the staged table and afterwards the history of `rowb`
// bytes a frame -- in LDS while all max_frames rows fit kTabLds, else in the
// caller's workspace with `spill` bytes of LDS beside it.
struct StringPlan {
  int P, stage_tab, hist_lds, lds;
  size_t ws;
};
inline void string_layout(const lt_graph* g, const lt_table_problem* pb, long long fixed,
                          long long rowb, long long spill, StringPlan* pl) {
  const long long stage = stage_table(g);
  pl->stage_tab = stage ? 1 : 0;
  const long long histb = rowb * pb->max_frames;
  pl->hist_lds = fixed + std::max(histb, stage) <= kTabLds ? 1 : 0;
  const long long region = std::max(pl->hist_lds ? histb : spill, stage);
  pl->lds = (int)(fixed + ((region + 15) & ~15LL));
  pl->ws = pl->hist_lds ? 0 : (size_t)(((long long)pb->batch * histb + 255) & ~255LL);
}

// The launch of kernel k: its dynamic LDS limit raised when needed. Errors
// read "<what> LDS" and "<what><what_launch>".
template <typename K, typename A>
int launch(K k, dim3 grid, dim3 block, int lds, hipStream_t st, const A& a, const char* what,
           const char* what_launch = " kernel launch") {
  if (lds > 64 * 1024)
    if (hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds) !=
        hipSuccess)
      return fail(LT_EHIP, std::string(what) + " LDS");
  hipLaunchKernelGGL(k, grid, block, lds, st, a);
  return hipGetLastError() == hipSuccess ? LT_OK : fail(LT_EHIP, std::string(what) + what_launch);
}

// f(std::bool_constant<BF16>) / f(std::bool_constant<BF16>, std::integral_constant<int, P>)
// for the runtime dtype and P in {1, 2, 4}.
template <typename F>
int dispatch(bool bf16, const F& f) {
  return bf16 ? f(std::true_type{}) : f(std::false_type{});
}
template <typename F>
int dispatch(bool bf16, int P, const F& f) {
  return dispatch(bf16, [&](auto bf) {
    if (P == 1) return f(bf, std::integral_constant<int, 1>{});
    if (P == 2) return f(bf, std::integral_constant<int, 2>{});
    return f(bf, std::integral_constant<int, 4>{});
  });
}

}  // namespace

#endif  // LT_STRING_COMMON_H_
