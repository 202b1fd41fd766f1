// lt_edit.hip -- unit-cost Levenshtein distance of hypotheses against
// references (lt_edit_distance, defined in include/lt_paths.h).
//
// One wave per (utterance, hypothesis). The DP row D[0..n] over the reference
// positions lives in registers, P consecutive cells a lane (lane l: cells
// l*P .. l*P + P-1); each hypothesis token h is one row update,
//   tmp[j] = min(D[j] + 1, D[j-1] + [ref_j != h])   D[j-1] of a lane's first
//                                                   cell by a one-lane shift
//   D'[j]  = j + min_{k <= j} (tmp[k] - k)          the insertion chain in
//                                                   closed form: a running min
//                                                   inside the lane, a DPP
//                                                   prefix-min scan over the
//                                                   lanes' totals, shifted by
//                                                   one lane
//   tokens  the reference's (values > 0 among the first num_labels) are
//           compacted once into an LDS row of the wave by ballot + popcount,
//           and each lane keeps its P cells' tokens in registers; the
//           hypothesis's come from 64-frame coalesced loads, a ballot of the
//           lanes > 0 and a loop over the set bits.
// Cells past n hold finite values nobody reads: a cell depends on lower cells
// only.
#include "lt_string_common.h"

namespace {

struct EArgs {
  const long long* hyp;  // [B, S, T]
  const int* nfr;        // [B] or null
  const int* ref;        // [B, U]
  const int* nlab;       // [B]
  int* dist;             // [B, S]
  int* hlen;             // [B, S] or null
  int B, S, T, U;
  int wpb;   // waves (hypotheses) per workgroup
  int nblk;  // workgroups per utterance
};

constexpr int kEditCells = 1024;  // most DP cells: 64 lanes of 16
constexpr int kEditBig = 0x7fffffff;

template <int CTRL, int ROW_MASK>
LT_DEVINL int dpp_min_into(int v) {
  // lanes without a source (or outside ROW_MASK) read the identity
  const int o = __builtin_amdgcn_update_dpp(kEditBig, v, CTRL, ROW_MASK, 0xF, false);
  return o < v ? o : v;
}

// min over the lanes below this one (the identity in lane 0)
LT_DEVINL int wave_prefix_min_exclusive(int v) {
  v = dpp_min_into<0x111, 0xF>(v);  // row_shr:1
  v = dpp_min_into<0x112, 0xF>(v);  // row_shr:2
  v = dpp_min_into<0x114, 0xF>(v);  // row_shr:4
  v = dpp_min_into<0x118, 0xF>(v);  // row_shr:8
  v = dpp_min_into<0x142, 0xA>(v);  // row_bcast:15 into rows 1 and 3
  v = dpp_min_into<0x143, 0xC>(v);  // row_bcast:31 into rows 2 and 3
  return __builtin_amdgcn_update_dpp(kEditBig, v, 0x138, 0xF, 0xF, false);  // wave_shr:1
}

template <int P>
__global__ __launch_bounds__(512) void edit_kernel(const EArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char e_sm[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x / a.nblk;
  const int s = (blockIdx.x % a.nblk) * a.wpb + wave;
  if (s >= a.S) return;  // wave-uniform; the kernel has no barrier
  const int T = a.T, U = a.U;
  int nf = a.nfr ? a.nfr[b] : T;
  nf = nf < 0 ? 0 : (nf > T ? T : nf);
  const int nl = a.nlab[b];
  const bool ranged = nl >= 0 && nl <= U;
  const long long* hyp = a.hyp + ((long long)b * a.S + s) * T;

  // the reference's tokens, compacted: rtok[j] is the token of cell j + 1
  int* rtok = (int*)e_sm + wave * (64 * P);
  int n = 0;
  if (ranged) {
    const int* ref = a.ref + (long long)b * U;
    for (int base = 0; base < nl; base += 64) {
      const int u = base + lane;
      const int r = u < nl ? ref[u] : 0;
      const unsigned long long m = __ballot(r > 0);
      if (r > 0) rtok[n + __popcll(m & ((1ull << lane) - 1))] = r;
      n += __popcll(m);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  n = __builtin_amdgcn_readfirstlane(n);

  int D[P], rj[P];
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int j = lane * P + i;
    D[i] = j;
    rj[i] = (j >= 1 && j <= n) ? rtok[j - 1] : 0;  // 0 matches no token
  }

  int count = 0;
  for (int base = 0; base < nf; base += 64) {
    const int t = base + lane;
    const long long y64 = t < nf ? hyp[t] : 0;
    // a token past int32 matches no reference token
    const int y = y64 > 0x7fffffffLL ? -1 : (int)y64;
    unsigned long long m = __ballot(y64 > 0);
    count += __popcll(m);
    if (!ranged) continue;
    for (; m; m &= m - 1) {
      const int h = __builtin_amdgcn_readlane(y, __ffsll((long long)m) - 1);
      // D[j-1] of the lane's first cell: the cell below, from the lane below
      int left = __builtin_amdgcn_update_dpp(kEditBig, D[P - 1], 0x138, 0xF, 0xF, false);
      int run = kEditBig;  // min of tmp[k] - k over the lane's cells so far
      int tmp[P];
#pragma unroll
      for (int i = 0; i < P; ++i) {
        const int j = lane * P + i;
        const int del = D[i] + 1;
        // cell 0 has no left neighbour (left is the identity in lane 0)
        const int sub = (j == 0) ? kEditBig : left + (rj[i] != h ? 1 : 0);
        const int v = (del < sub ? del : sub) - j;
        run = v < run ? v : run;
        tmp[i] = run;
        left = D[i];
      }
      const int below = wave_prefix_min_exclusive(run);
#pragma unroll
      for (int i = 0; i < P; ++i) {
        const int j = lane * P + i;
        D[i] = j + (below < tmp[i] ? below : tmp[i]);
      }
    }
  }

  int d = -1;
  if (ranged) {
    int mine = D[0];
#pragma unroll
    for (int i = 1; i < P; ++i) mine = (n % P) == i ? D[i] : mine;
    d = __builtin_amdgcn_readlane(mine, n / P);
  }
  if (lane == 0) {
    a.dist[(long long)b * a.S + s] = d;
    if (a.hlen) a.hlen[(long long)b * a.S + s] = count;
  }
}

template <int P>
int edit_launch(const EArgs& a, hipStream_t st) {
  const int lds = a.wpb * 64 * P * 4;  // at most 32 KiB
  return launch(edit_kernel<P>, dim3((unsigned)(a.B * a.nblk)), dim3(64 * a.wpb), lds, st, a,
                "edit distance");
}

}  // namespace

extern "C" {

int lt_edit_distance(int32_t batch, int32_t num_hyps, int32_t max_frames, int32_t max_labels,
                     const int64_t* hyp, const int32_t* num_frames, const int32_t* ref,
                     const int32_t* num_labels, int32_t* distance, int32_t* hyp_length,
                     void* stream) {
  if (batch < 0 || max_frames < 0 || max_labels < 0)
    return fail(LT_EINVAL, "lt_edit_distance: negative shape");
  if (num_hyps < 1) return fail(LT_EINVAL, "lt_edit_distance: num_hyps < 1");
  if ((long long)max_labels + 1 > kEditCells)
    return fail(LT_EUNSUPPORTED, "lt_edit_distance: max_labels > 1023");
  if ((long long)num_hyps * batch > 0x7fffffffLL)
    return fail(LT_EUNSUPPORTED, "lt_edit_distance: 2^31 hypotheses or more");
  if (batch == 0) return LT_OK;
  if (!distance || !num_labels || (!hyp && max_frames > 0) || (!ref && max_labels > 0))
    return fail(LT_EINVAL, "lt_edit_distance: null pointer");
  if (((uintptr_t)hyp & 7) || ((uintptr_t)num_frames & 3) || ((uintptr_t)ref & 3) ||
      ((uintptr_t)num_labels & 3) || ((uintptr_t)distance & 3) || ((uintptr_t)hyp_length & 3))
    return fail(LT_EINVAL, "misaligned pointer");
  EArgs a;
  memset(&a, 0, sizeof(a));
  a.hyp = (const long long*)hyp;
  a.nfr = num_frames;
  a.ref = ref;
  a.nlab = num_labels;
  a.dist = distance;
  a.hlen = hyp_length;
  a.B = batch;
  a.S = num_hyps;
  a.T = max_frames;
  a.U = max_labels;
  a.wpb = num_hyps < 8 ? num_hyps : 8;
  a.nblk = (num_hyps + a.wpb - 1) / a.wpb;
  hipStream_t st = (hipStream_t)stream;
  const int cells = max_labels + 1;
  if (cells <= 64) return edit_launch<1>(a, st);
  if (cells <= 128) return edit_launch<2>(a, st);
  if (cells <= 256) return edit_launch<4>(a, st);
  if (cells <= 512) return edit_launch<8>(a, st);
  return edit_launch<16>(a, st);
}

}  // extern "C"
