// lt_beam_joint.hip -- prefix beam search with the joint weight function
// fused in (include/lt_beam_joint.h): the search of lt_beam.hip on
//   W[b, t, c, y] = bias[y] + sum_h Wo[y, h] * tanh(Pc[c, h] + Pf[b*T + t, h])
// where W is never written. A beam of K slots reads K of a frame's C rows, so
// per frame only those rows are formed, on v_mfma_f32_32x32x16_bf16 through
// joint_tile (lt_joint.h) -- the producer's K steps in the producer's order, so
// the rows are lt_joint_weights_ex's bit for bit -- into a [64][R] fp32 tile in
// LDS, row = slot, which beam_frame (lt_beam_common.h) searches.
//
// One workgroup of 8 waves per utterance:
//   wave 0      the search: lane r is slot r, as in lt_beam.hip.
//   waves 1..4  the producers: wave 1 + 2 rt + ct forms rows [32 rt, 32 rt + 32)
//               x columns [32 ct, 32 ct + 32) of the tile. A tile whose rows
//               are all dead slots, or whose columns are past R, is skipped,
//               so 1 (K <= 32, R <= 32) to 4 waves work. H is not split over
//               waves: that would change the order of the sums.
//   waves 5..7  the stagers: e^{2 Pf[t]} rows (the producer's exp2x, so the
//               operands are bit-equal) and each frame's |Pf| > 40 flag, one
//               slice of L frames ahead into a two-slice LDS ring, a frame
//               row per wave. A frame over 40 (or a call whose Pc is) keeps Pf
//               itself: the producers then take joint_tile's direct path.
// The frame's chain, two workgroup barriers:
//   wave 0 publishes the slots' context states and the live count   | barrier
//   the producers gather e^{2 Pc[c_slot]} (from LDS when the table
//   fits there, else from the workspace: read-mostly, L2-resident),
//   run joint_tile, add the bias, write the tile                      | barrier
//   wave 0 searches the tile (merge, select, new beam, trace row).
// Wo (bf16 hi, and lo for split products, rows padded as the producer pads
// them) is staged once, the next-state table and e^{2 Pc} when they fit.
#include "lt_beam_common.h"
#include "lt_joint.h"

namespace {

constexpr int kJbThreads = 512;
constexpr int kJbFlags = 256;          // per-block |Pc| > 40 flags of the pre-pass
constexpr int kJbMaxH = 1024;          // a stager lane holds a frame row in 4 float4
constexpr int kJbLds = 160 * 1024 - 512;  // dynamic LDS: the CU's, less the barrier-reduce words
// largest e^{2 Pc} table staged in LDS: the bigram's at hidden = 512 (66 KiB)
constexpr long long kJbStageEc = 72 * 1024;

struct JbArgs {
  BArgs b;           // the search's arguments (W unused)
  const float* pc;   // [C, H]
  const float* pf;   // [B*T, H]
  const float* ec;   // [C, H] e^{2 pc} (workspace)
  const int* big;    // [kJbFlags] != 0: some |pc| > kSplitMax
  const float* wo;   // [R, H]
  const float* bias; // [R]
  int H, L, stage_ec;
  int o_tile, o_ring, o_flag, o_cst, o_mrows, o_sbuf, o_tab, o_ec;  // LDS byte offsets
};

// e^{2 pc} and, per block, whether any |pc| > kSplitMax (NaN counts). Every
// one of the kJbFlags words is written: no memset.
__global__ __launch_bounds__(256) void jbeam_exp_kernel(const float* pc, float* ec, int* flags,
                                                        long long n4) {
  bool over = false;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4;
       i += (long long)gridDim.x * 256) {
    const float4 x = ((const float4*)pc)[i];
    const float m = fmaxf(fmaxf(fabsf(x.x), fabsf(x.y)), fmaxf(fabsf(x.z), fabsf(x.w)));
    over |= !(m <= kSplitMax);
    const f32x2 lo = exp2x(f32x2{x.x, x.y}), hi = exp2x(f32x2{x.z, x.w});
    ((float4*)ec)[i] = float4{lo.x, lo.y, hi.x, hi.y};
  }
  const int any = __syncthreads_or(over);
  if (threadIdx.x == 0) flags[blockIdx.x] = any;
  if (blockIdx.x == 0)
    for (int j = gridDim.x + threadIdx.x; j < kJbFlags; j += 256) flags[j] = 0;
}

template <int MODE, bool SP>
__global__ __launch_bounds__(kJbThreads) void joint_beam_kernel(const JbArgs ja) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_sm[];
  const BArgs& a = ja.b;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x;
  const int T = a.T, K = a.K, R = a.R, H = ja.H, L = ja.L;
  const int HP = H + 8, WL = (R * HP + 7) & ~7, h4 = H / 4;
  int nf = a.nfr[b];
  nf = nf < 0 ? 0 : (nf > T ? T : nf);

  unsigned short* wol = (unsigned short*)s_sm;       // [R][HP] bf16 hi (, lo)
  float* tile = (float*)(s_sm + ja.o_tile);          // [64][R] the beam's weight rows
  float* ring = (float*)(s_sm + ja.o_ring);          // [2][L][H] e^{2 pf} (or pf)
  int* flag = (int*)(s_sm + ja.o_flag);              // [2][L] the frame takes the direct path
  int* cst = (int*)(s_sm + ja.o_cst);                // [64] the slots' states, [64]: live slots
  unsigned* mrows = (unsigned*)(s_sm + ja.o_mrows);  // [64, MW]
  float4* sbuf = (float4*)(s_sm + ja.o_sbuf);        // [64]
  int* tab = (int*)(s_sm + ja.o_tab);
  float* ecl = (float*)(s_sm + ja.o_ec);
  const LaneDeal ld = {lane / R, lane % R, 64 / R, 64 % R};

  stage_wo<SP>(ja.wo, wol, R, H, HP, WL, tid, kJbThreads);
  if (a.stage_tab)
    for (int i = tid; i < a.C * a.V; i += kJbThreads) tab[i] = a.table[i];
  if (ja.stage_ec)
    for (int i = tid; i < a.C * h4; i += kJbThreads) ((float4*)ecl)[i] = ((const float4*)ja.ec)[i];
  const int* tbl = a.stage_tab ? tab : a.table;
  const bool cbig = __syncthreads_or(tid < kJbFlags ? ja.big[tid] : 0);

  // padding frames of the trace outputs
  const long long tr0 = (long long)b * T * K;
  for (long long i = (long long)nf * K + tid; i < (long long)T * K; i += kJbThreads) {
    if (a.pad_trace) a.trace[tr0 + i] = -1;
    if (a.step) a.step[tr0 + i] = -kInf;
  }

  // stager wave sw of 3: the frame rows sw, sw + 3, ... of slice i
  auto stage_slice = [&](int i, int sw) {
    const int ta = i * L, tb = ta + L < nf ? ta + L : nf;
    for (int t = ta + sw; t < tb; t += 3) {
      const float4* src = (const float4*)(ja.pf + ((long long)b * T + t) * H);
      const float4 z4 = {0.f, 0.f, 0.f, 0.f};
      float4 v[4];
      bool over = false;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        v[u] = lane + 64 * u < h4 ? src[lane + 64 * u] : z4;
        const float m =
            fmaxf(fmaxf(fabsf(v[u].x), fabsf(v[u].y)), fmaxf(fabsf(v[u].z), fabsf(v[u].w)));
        over |= !(m <= kSplitMax);  // NaN counts as over
      }
      const bool direct = cbig || __any(over);
      const int fi = (i & 1) * L + (t - ta);
      float4* dst = (float4*)(ring + (long long)fi * H);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (lane + 64 * u >= h4) continue;
        if (direct) {
          dst[lane + 64 * u] = v[u];
        } else {
          const f32x2 lo = exp2x(f32x2{v[u].x, v[u].y}), hi = exp2x(f32x2{v[u].z, v[u].w});
          dst[lane + 64 * u] = float4{lo.x, lo.y, hi.x, hi.y};
        }
      }
      if (lane == 0) flag[fi] = direct;
    }
  };

  // the producers' constants: wave 1 + 2 rt + ct, lane row / column r, K half hk
  const int pt = wave - 1, rt = pt >> 1, ct = pt & 1;
  const int r = lane & 31, half = lane >> 5, hk = 8 * half;
  const int y = 32 * ct + r;
  const bool vy = y < R;
  const bool is_prod = wave >= 1 && wave <= 4 && 32 * ct < R;
  const float by = is_prod && vy ? ja.bias[y] : 0.f;
  // columns past R read row R - 1 (valid) and are never stored
  const unsigned short* w0 = wol + (vy ? y : R - 1) * HP + hk;
  const unsigned short* w0l = w0 + WL;

  const int nsl = (nf + L - 1) / L;
  if (wave >= 5 && nsl > 0) stage_slice(0, wave - 5);
  Slot q = {lane == 0 ? 0.f : -kInf, 0, 0, 0, 0ull, 0ull};
  int nlive = 1;
  if (wave == 0) {
    cst[lane] = 0;
    if (lane == 0) cst[64] = 1;
  }
  __syncthreads();  // Wo, the tables, slice 0, the first beam's states
  for (int i = 0; i < nsl; ++i) {
    const int ta = i * L, tb = ta + L < nf ? ta + L : nf;
    // slice i + 1 goes to the half that slice i - 1 was read from
    if (wave >= 5 && i + 1 < nsl) stage_slice(i + 1, wave - 5);
    for (int t = ta; t < tb; ++t) {
      if (is_prod && 32 * rt < cst[64]) {
        const int fi = (i & 1) * L + (t - ta);
        const bool split = flag[fi] == 0;
        const long long co = (long long)cst[32 * rt + r] * H + hk;
        const float* pfr = ring + (long long)fi * H + hk;
        f32x16 acc = {}, none = {};
        if (!split)
          joint_tile<SP, false>(false, ja.pc + co, pfr, H, w0, w0, w0l, w0l, acc, none);
        else if (ja.stage_ec)
          joint_tile<SP, false>(true, ecl + co, pfr, H, w0, w0, w0l, w0l, acc, none);
        else
          joint_tile<SP, false>(true, ja.ec + co, pfr, H, w0, w0, w0l, w0l, acc, none);
        // C/D: column y, row (j & 3) + 8 (j >> 2) + 4 half of the row tile
        if (vy) {
#pragma unroll
          for (int j = 0; j < 16; ++j)
            tile[(32 * rt + (j & 3) + 8 * (j >> 2) + 4 * half) * R + y] = acc[j] + by;
        }
      }
      __syncthreads();  // the tile of frame t
      if (wave == 0) {
        beam_frame<MODE, false, true>(q, nlive, (const unsigned char*)tile, mrows, sbuf, tbl, a,
                                      ld, lane, tr0 + (long long)t * K);
        cst[lane] = lane < nlive ? q.c : 0;
        if (lane == 0) cst[64] = nlive;
      }
      __syncthreads();  // the next beam's states; the tile is free
    }
  }
  if (wave == 0) beam_finish(q, nlive, a, b, nf, lane, tr0);
}

struct JbPlan {
  int L, MW, stage_tab, stage_ec, lds;
  int o_tile, o_ring, o_flag, o_cst, o_mrows, o_sbuf, o_tab, o_ec;
  size_t ec_bytes, trace_bytes;
};

constexpr size_t kJbFlagBytes = 4 * kJbFlags;

// Validates the shape and lays out the workgroup's LDS.
int jbeam_plan(const lt_graph* g, const lt_table_problem* pb, const lt_joint_params* jp,
               int beam_size, JbPlan* pl) {
  if (!jp) return fail(LT_EINVAL, "lt_joint_beam_search: null joint parameters");
  if (int rc = table_check("lt_joint_beam_search", g, pb, 0, [&] {
        if (beam_size < 1) return fail(LT_EINVAL, "lt_joint_beam_search: beam_size < 1");
        if (jp->hidden < 1) return fail(LT_EINVAL, "lt_joint_beam_search: hidden < 1");
        if (jp->precision != LT_JOINT_BF16 && jp->precision != LT_JOINT_SPLIT)
          return fail(LT_EINVAL,
                      "lt_joint_beam_search: precision must be LT_JOINT_BF16 or LT_JOINT_SPLIT");
        if (g->expansions >= 1)
          return fail(LT_EUNSUPPORTED, "lt_joint_beam_search: FrameLabelDependent is not searched");
        if (int rc = check_arrays(g, false)) return rc;
        if (beam_size > kBeamMaxK)
          return fail(LT_EUNSUPPORTED, "lt_joint_beam_search: beam_size > 64 (one wave)");
        if (g->vocab_size + 1 > 64)
          return fail(LT_EUNSUPPORTED, "lt_joint_beam_search: V + 1 > 64 (two column tiles)");
        if (jp->hidden % 16 || jp->hidden > kJbMaxH)
          return fail(LT_EUNSUPPORTED,
                      "lt_joint_beam_search: needs hidden % 16 == 0, hidden <= 1024");
        if (pb->weight_dtype != LT_DTYPE_F32)
          return fail(LT_EUNSUPPORTED, "lt_joint_beam_search: the weights are fp32");
        return LT_OK;
      }))
    return rc;
  const long long C = g->num_states, R = g->vocab_size + 1, H = jp->hidden;
  const long long ntrace = (long long)pb->batch * pb->max_frames * beam_size;
  if (ntrace > 0x7fffffffLL)
    return fail(LT_EUNSUPPORTED, "lt_joint_beam_search: a trace of 2^31 elements or more");
  pl->trace_bytes = (size_t)ntrace * 4;
  pl->ec_bytes = (size_t)(4 * C * H);
  pl->MW = (int)((R + 31) / 32);
  const bool sp = jp->precision == LT_JOINT_SPLIT;
  auto up16 = [](long long x) { return (x + 15) & ~15LL; };
  const long long wob = up16((sp ? 4LL : 2LL) * ((R * (H + 8) + 7) & ~7LL));
  const long long tileb = up16(64 * R * 4), cstb = up16(65 * 4);
  const long long mrb = 64LL * pl->MW * 4, sbb = 64 * 16;
  const long long fixed = wob + tileb + cstb + mrb + sbb;
  // the ring: two slices of L frames, L as large as fits up to 8, at least 1
  long long L = 8;
  auto ringb = [&](long long l) { return 2 * l * H * 4 + up16(2 * l * 4); };
  while (L > 1 && fixed + ringb(L) > kJbLds) L >>= 1;
  if (fixed + ringb(L) > kJbLds)
    return fail(LT_EUNSUPPORTED, "lt_joint_beam_search: the output projection, the weight tile "
                                 "and the frame ring exceed the CU's 160 KB of LDS");
  long long tabb = up16(stage_table(g));
  if (fixed + ringb(L) + tabb > kJbLds) tabb = 0;
  // e^{2 Pc} in LDS when it fits beside them, at the price of a shorter ring
  // (the stagers are a slice ahead either way) down to 2 frames a slice
  const long long ecb = 4 * C * H;
  long long Le = L;
  while (Le > 2 && fixed + ringb(Le) + tabb + ecb > kJbLds) Le >>= 1;
  pl->stage_ec = ecb <= kJbStageEc && fixed + ringb(Le) + tabb + ecb <= kJbLds ? 1 : 0;
  if (pl->stage_ec) L = Le;
  pl->stage_tab = tabb ? 1 : 0;
  pl->L = (int)L;
  pl->o_tile = (int)wob;
  pl->o_ring = pl->o_tile + (int)tileb;
  pl->o_flag = pl->o_ring + (int)(2 * L * H * 4);
  pl->o_cst = pl->o_flag + (int)up16(2 * L * 4);
  pl->o_mrows = pl->o_cst + (int)cstb;
  pl->o_sbuf = pl->o_mrows + (int)mrb;
  pl->o_tab = pl->o_sbuf + (int)sbb;
  pl->o_ec = pl->o_tab + (int)tabb;
  const long long lds = fixed + ringb(L) + tabb + (pl->stage_ec ? ecb : 0);
  pl->lds = (int)lds;
  return LT_OK;
}

}  // namespace

extern "C" {

int lt_joint_beam_search_workspace_bytes(const lt_graph* g, const lt_table_problem* pb,
                                         const lt_joint_params* jp, int32_t beam_size,
                                         size_t* bytes) {
  JbPlan pl;
  if (int rc = jbeam_plan(g, pb, jp, beam_size, &pl)) return rc;
  if (bytes) *bytes = kJbFlagBytes + pl.ec_bytes + pl.trace_bytes;
  return LT_OK;
}

int lt_joint_beam_search(const lt_graph* g, const lt_table_problem* pb, const lt_joint_params* jp,
                         const int32_t* num_frames, int32_t beam_size, int32_t semiring,
                         int64_t* labels, int32_t* num_labels, float* scores, int32_t* trace,
                         float* step_score, void* workspace, size_t workspace_bytes,
                         void* stream) {
  JbPlan pl;
  if (int rc = jbeam_plan(g, pb, jp, beam_size, &pl)) return rc;
  if (semiring != LT_SEMIRING_LOG && semiring != LT_SEMIRING_MAX)
    return fail(LT_EINVAL, "lt_joint_beam_search: the semiring is Log or MaxTropical");
  if (!num_labels || !scores || (!labels && pb->max_frames > 0))
    return fail(LT_EINVAL, "lt_joint_beam_search: null output");
  if (pb->batch == 0) return LT_OK;
  if (!num_frames || !jp->ctx_proj || !jp->out_weight || !jp->out_bias ||
      (!jp->frame_proj && pb->max_frames > 0))
    return fail(LT_EINVAL, "lt_joint_beam_search: null pointer");
  const size_t need = kJbFlagBytes + pl.ec_bytes + (trace ? 0 : pl.trace_bytes);
  if (!workspace || workspace_bytes < need)
    return fail(LT_EINVAL, "lt_joint_beam_search: workspace too small");
  if (((uintptr_t)jp->ctx_proj & 15) || ((uintptr_t)jp->frame_proj & 15) ||
      ((uintptr_t)workspace & 15) || ((uintptr_t)jp->out_weight & 3) ||
      ((uintptr_t)jp->out_bias & 3) || ((uintptr_t)num_frames & 3) || ((uintptr_t)labels & 7) ||
      ((uintptr_t)num_labels & 3) || ((uintptr_t)scores & 3) || ((uintptr_t)trace & 3) ||
      ((uintptr_t)step_score & 3))
    return fail(LT_EINVAL, "lt_joint_beam_search: misaligned pointer");
  char* ws = (char*)workspace;
  int* flags = (int*)ws;
  float* ec = (float*)(ws + kJbFlagBytes);
  JbArgs ja;
  memset(&ja, 0, sizeof(ja));
  BArgs& a = ja.b;
  a.nfr = num_frames;
  a.table = g->next_state;
  a.labels = (long long*)labels;
  a.nlab = num_labels;
  a.scores = scores;
  a.trace = trace ? trace : (int*)(ws + kJbFlagBytes + pl.ec_bytes);
  a.pad_trace = trace ? 1 : 0;
  a.step = step_score;
  a.B = pb->batch;
  a.T = pb->max_frames;
  a.C = g->num_states;
  a.V = g->vocab_size;
  a.R = g->vocab_size + 1;
  a.K = beam_size;
  a.MW = pl.MW;
  a.stage_tab = pl.stage_tab;
  ja.pc = jp->ctx_proj;
  ja.pf = jp->frame_proj;
  ja.ec = ec;
  ja.big = flags;
  ja.wo = jp->out_weight;
  ja.bias = jp->out_bias;
  ja.H = jp->hidden;
  ja.L = pl.L;
  ja.stage_ec = pl.stage_ec;
  ja.o_tile = pl.o_tile; ja.o_ring = pl.o_ring; ja.o_flag = pl.o_flag; ja.o_cst = pl.o_cst;
  ja.o_mrows = pl.o_mrows; ja.o_sbuf = pl.o_sbuf; ja.o_tab = pl.o_tab; ja.o_ec = pl.o_ec;
  hipStream_t st = (hipStream_t)stream;
  const long long n4 = (long long)a.C * ja.H / 4;
  const int grid = (int)std::max<long long>(1, std::min<long long>((n4 + 255) / 256, kJbFlags));
  hipLaunchKernelGGL(jbeam_exp_kernel, dim3(grid), dim3(256), 0, st, ja.pc, ec, flags, n4);
  if (hipGetLastError() != hipSuccess)
    return fail(LT_EHIP, "lt_joint_beam_search: pre-pass kernel launch");
  const bool sp = jp->precision == LT_JOINT_SPLIT;
  auto k = semiring == LT_SEMIRING_LOG
               ? (sp ? joint_beam_kernel<M_LOG, true> : joint_beam_kernel<M_LOG, false>)
               : (sp ? joint_beam_kernel<M_MAX, true> : joint_beam_kernel<M_MAX, false>);
  return launch(k, dim3((unsigned)a.B), dim3(kJbThreads), pl.lds, st, ja, "joint beam search");
}

}  // extern "C"
