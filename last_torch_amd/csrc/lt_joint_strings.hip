// lt_joint_strings.hip -- the rows of the joint weight function's W that a
// label string visits (include/lt_joint_strings.h):
//   Ws[b, t, k, y] = bias[y] + sum_h Wo[y, h] * tanh(Pc[s_k(b), h] + Pf[b*T + t, h])
// s_k the context state after the first k non-epsilon labels of utterance b.
// The string kernels (lt_align.hip, lt_align_long.hip, lt_align_post.hip,
// lt_align_post_long.hip) read W in those rows only, so on the chain table
// (state k -> min(k + 1, U) on every label) and Ws they read what they would
// read on the model's table and W [B, T, C, V+1], which is never formed.
//
// Two launches:
//   jstr_walk_kernel  one workgroup per utterance: the labels to LDS, one
//       thread walks the model's table as string_prologue does, s_k and n_b
//       (the number of non-epsilon labels) out, then all threads gather the
//       visited rows e^{2 Pc[s_k]} [B, U+1, H] into the workspace -- or Pc[s_k]
//       itself when one of the utterance's visited rows exceeds 40 (the flag).
//   jstr_rows_kernel  the producer. A tile is 32 consecutive chain rows of one
//       frame by all V+1 columns: one contiguous run of 32 (V+1) values of Ws.
//       A workgroup takes (utterance, row tile, frame slice): Wo (bf16 hi, lo
//       for split products) and the tile's 32 context rows go to LDS once, and
//       its waves walk the slice's frames -- the producer's frame-block kernel
//       (lt_producer.hip) with the roles of frames and context states swapped.
//       A wave loads frame t + nw's row while it works on frame t, turns it
//       into e^{2 Pf} in a private LDS row that all its lanes read (broadcast),
//       runs joint_tile (lt_joint.h: the producer's K steps in the producer's
//       order), adds the bias and stores as the producer stores. Tiles past
//       n_b and frames past num_frames are zero stores without tanh work.
// When the 32 context rows do not fit LDS beside Wo (V + 1 = 33, split
// products: past hidden = 576), the lanes read their rows from the gathered
// image in the workspace instead.
#include "lt_string_common.h"
#include "lt_joint.h"

namespace {

constexpr int kJsWalkThreads = 256;
constexpr int kJsMaxU = 4095;
constexpr int kJsMaxH = 1024;          // a lane holds a frame row in 4 float4
constexpr int kJsLds = 160 * 1024;
// largest next-state table the walk stages beside its 32 KB of labels and
// states: the workgroup stays within the 64 KB a launch has by default
constexpr long long kJsStageTab = 16 * 1024;

struct JsArgs {
  const int* table;   // [C, V]
  const int* labels;  // [B, U]
  const int* nfr;     // [B]
  const float* pc;    // [C, H]
  const float* pf;    // [B*T, H]
  const float* wo;    // [R, H]
  const float* bias;  // [R]
  void* Ws;           // [B, T, U+1, R]
  int* states;        // [B, U+1] or null
  int* hdr;           // workspace: [B] over-40 flags, [B] n_b
  int* st;            // workspace: [B, U+1] s_k (k <= n_b written)
  float* rows;        // workspace: [B, U+1, H] e^{2 Pc[s_k]} or Pc[s_k] (k <= n_b written)
  int B, T, U, C, V, R, H;
  int NT, S, FL;      // row tiles; frame slices per (b, tile); frames per slice
  int nw, stage_ctx, stage_tab;
  int o_ctx, o_crow;  // LDS byte offsets of the producer
};

__global__ __launch_bounds__(kJsWalkThreads) void jstr_walk_kernel(const JsArgs a) {
  extern __shared__ __attribute__((aligned(16))) int s_tab[];  // the table when it is small
  __shared__ int yt[kJsMaxU + 1];
  __shared__ int st[kJsMaxU + 1];
  __shared__ int s_n;
  const int tid = threadIdx.x, b = blockIdx.x;
  const int U = a.U, U1 = U + 1, h4 = a.H / 4;
  for (int u = tid; u < U; u += kJsWalkThreads) {
    int y = a.labels[(long long)b * U + u];
    if (y < 0 || y > a.V) y = 0;
    yt[u] = y;
  }
  if (a.stage_tab)
    for (int i = tid; i < a.C * a.V; i += kJsWalkThreads) s_tab[i] = a.table[i];
  __syncthreads();
  if (tid == 0) {
    auto walk = [&](const int* tb) {
      int c = 0, k = 0;
      st[0] = 0;
      for (int u = 0; u < U; ++u) {
        const int y = yt[u];
        if (y != 0) {
          c = tb[c * a.V + y - 1];
          st[++k] = c;
        }
      }
      s_n = k;
    };
    if (a.stage_tab) walk(s_tab);
    else walk(a.table);
  }
  __syncthreads();
  const int n = s_n;
  for (int k = tid; k < U1; k += kJsWalkThreads) {
    if (a.states) a.states[(long long)b * U1 + k] = k <= n ? st[k] : -1;
    if (k <= n) a.st[(long long)b * U1 + k] = st[k];
  }
  // the visited rows: over 40 (or NaN) anywhere keeps the utterance's rows raw
  const float4* pc4 = (const float4*)a.pc;
  bool over = false;
  for (int i = tid; i < (n + 1) * h4; i += kJsWalkThreads) {
    const int k = i / h4, j = i - k * h4;
    const float4 x = pc4[(long long)st[k] * h4 + j];
    const float m = fmaxf(fmaxf(fabsf(x.x), fabsf(x.y)), fmaxf(fabsf(x.z), fabsf(x.w)));
    over |= !(m <= kSplitMax);
  }
  const bool big = __syncthreads_or(over);
  float4* dst = (float4*)a.rows + (long long)b * U1 * h4;
  for (int i = tid; i < (n + 1) * h4; i += kJsWalkThreads) {
    const int k = i / h4, j = i - k * h4;
    const float4 x = pc4[(long long)st[k] * h4 + j];
    if (big) {
      dst[i] = x;
    } else {
      const f32x2 lo = exp2x(f32x2{x.x, x.y}), hi = exp2x(f32x2{x.z, x.w});
      dst[i] = float4{lo.x, lo.y, hi.x, hi.y};
    }
  }
  if (tid == 0) {
    a.hdr[b] = big;
    a.hdr[a.B + b] = n;
  }
}

template <bool OBF16, bool TWO, bool SP>
__global__ __launch_bounds__(1024) void jstr_rows_kernel(const JsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned short wsl[];  // [R][H + 8] bf16 (x2: SP)
  const int tid = threadIdx.x, lane = tid & 63, nthr = blockDim.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nw = a.nw;
  const int H = a.H, R = a.R, T = a.T, U1 = a.U + 1, HP = H + 8, FS = H + 4, h4 = H / 4;
  const int WL = (R * HP + 7) & ~7;  // SP: the lo block's offset
  const int s = blockIdx.x % a.S, q = blockIdx.x / a.S;
  const int rt = q % a.NT, b = q / a.NT;
  const int row0 = 32 * rt, nrow = U1 - row0 < 32 ? U1 - row0 : 32;
  const int t0 = s * a.FL, t1 = t0 + a.FL < T ? t0 + a.FL : T;
  int nf = a.nfr[b];
  nf = nf < 0 ? 0 : (nf > T ? T : nf);
  const int n = a.hdr[a.B + b];
  const bool ubig = a.hdr[b] != 0;
  // frames [t0, tl) of this tile are formed, [tl, t1) are zeros
  const int tl = row0 > n ? t0 : (nf < t0 ? t0 : (nf < t1 ? nf : t1));
  const long long bt = (long long)b * T;
  {
    const long long per = (long long)nrow * R, nz = (long long)(t1 - tl) * per;
    for (long long e = tid; e < nz; e += nthr) {
      const long long t = tl + e / per;
      stw<OBF16>(a.Ws, ((bt + t) * U1 + row0) * R + e % per, 0.f);
    }
  }
  if (tl == t0) return;

  float* ctl = (float*)((unsigned char*)wsl + a.o_ctx);                 // [32][H + 4]
  float* crow = (float*)((unsigned char*)wsl + a.o_crow) + wave * H;    // [nw][H]
  stage_wo<SP>(a.wo, wsl, R, H, HP, WL, tid, nthr);
  const float* grows = a.rows + (long long)b * U1 * H;
  if (a.stage_ctx)
    for (int e = tid; e < 32 * h4; e += nthr) {
      const int m = e / h4, k4 = e - m * h4;
      const int row = row0 + m < n ? row0 + m : n;  // dead rows read row n_b, never stored
      *(float4*)(ctl + m * FS + 4 * k4) = ((const float4*)(grows + (long long)row * H))[k4];
    }
  __syncthreads();

  const int r = lane & 31, half = lane >> 5, hk = 8 * half;
  const int y0 = r, y1 = 32 + r;
  const bool v0 = y0 < R, v1 = y1 < R;
  const float b0 = v0 ? a.bias[y0] : 0.f, b1 = v1 ? a.bias[y1] : 0.f;
  // columns past R read row R - 1 (valid) and are never stored
  const unsigned short* w0 = wsl + (v0 ? y0 : R - 1) * HP + hk;
  const unsigned short* w1 = wsl + (v1 ? y1 : R - 1) * HP + hk;
  const unsigned short* w0l = w0 + WL;
  const unsigned short* w1l = w1 + WL;
  const int rowl = row0 + r < n ? row0 + r : n;
  const float* gat = grows + (long long)rowl * H + hk;   // the lane's gathered row
  const float* ctr = ctl + r * FS + hk;                  // the same in LDS
  // a frame over 40 on an utterance whose rows are e^{2 Pc}: Pc itself
  const float* raw = ubig ? gat : a.pc + (long long)a.st[(long long)b * U1 + rowl] * H + hk;

  float4 p0, p1, p2, p3;
  const float4 z4 = {0.f, 0.f, 0.f, 0.f};
  auto load_row = [&](int t) {
    const float4* src = (const float4*)(a.pf + (bt + t) * H);
    p0 = lane < h4 ? src[lane] : z4;
    p1 = lane + 64 < h4 ? src[lane + 64] : z4;
    p2 = lane + 128 < h4 ? src[lane + 128] : z4;
    p3 = lane + 192 < h4 ? src[lane + 192] : z4;
  };
  auto amax = [](float4 v) {
    return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
  };
  auto e4 = [](float4 v) {
    const f32x2 lo = exp2x(f32x2{v.x, v.y}), hi = exp2x(f32x2{v.z, v.w});
    return float4{lo.x, lo.y, hi.x, hi.y};
  };
  if (t0 + wave < tl) load_row(t0 + wave);
  for (int t = t0 + wave; t < tl; t += nw) {
    const float m = fmaxf(fmaxf(amax(p0), amax(p1)), fmaxf(amax(p2), amax(p3)));
    const bool direct = ubig || __any(!(m <= kSplitMax));  // NaN counts as over
    float4* cw = (float4*)crow;
    if (lane < h4) cw[lane] = direct ? p0 : e4(p0);
    if (lane + 64 < h4) cw[lane + 64] = direct ? p1 : e4(p1);
    if (lane + 128 < h4) cw[lane + 128] = direct ? p2 : e4(p2);
    if (lane + 192 < h4) cw[lane + 192] = direct ? p3 : e4(p3);
    if (t + nw < tl) load_row(t + nw);
    const float* fr = crow + hk;
    f32x16 acc0 = {}, acc1 = {};
    if (direct)
      joint_tile<SP, TWO>(false, raw, fr, H, w0, w1, w0l, w1l, acc0, acc1);
    else if (a.stage_ctx)
      joint_tile<SP, TWO>(true, ctr, fr, H, w0, w1, w0l, w1l, acc0, acc1);
    else
      joint_tile<SP, TWO>(true, gat, fr, H, w0, w1, w0l, w1l, acc0, acc1);
    // C/D: column y = lane & 31 (+32), chain row (i & 3) + 8 (i >> 2) + 4 half
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = row0 + (i & 3) + 8 * (i >> 2) + 4 * half;
      if (row >= U1) continue;
      const bool live = row <= n;
      const long long o = ((bt + t) * U1 + row) * R;
      if (v0) stw<OBF16>(a.Ws, o + y0, live ? acc0[i] + b0 : 0.f);
      if (TWO && v1) stw<OBF16>(a.Ws, o + y1, live ? acc1[i] + b1 : 0.f);
    }
  }
}

struct JsPlan {
  int nw, stage_ctx, stage_tab, lds, o_ctx, o_crow;
  size_t hdr_bytes, st_bytes, row_bytes;
};

// Validates the shape and lays out the producer's LDS.
int jstr_plan(const lt_graph* g, const lt_table_problem* pb, const lt_joint_params* jp,
              JsPlan* pl) {
  if (!jp) return fail(LT_EINVAL, "lt_joint_string_rows: null joint parameters");
  if (int rc = table_check("lt_joint_string_rows", g, pb, kChkString, [&] {
        if (jp->hidden < 1) return fail(LT_EINVAL, "lt_joint_string_rows: hidden < 1");
        if (jp->precision != LT_JOINT_BF16 && jp->precision != LT_JOINT_SPLIT)
          return fail(LT_EINVAL,
                      "lt_joint_string_rows: precision must be LT_JOINT_BF16 or LT_JOINT_SPLIT");
        if (g->expansions >= 1)
          return fail(LT_EUNSUPPORTED, "lt_joint_string_rows: FrameLabelDependent is not served");
        if (g->vocab_size + 1 > 64)
          return fail(LT_EUNSUPPORTED, "lt_joint_string_rows: V + 1 > 64 (two column tiles)");
        if (jp->hidden % 16 || jp->hidden > kJsMaxH)
          return fail(LT_EUNSUPPORTED,
                      "lt_joint_string_rows: needs hidden % 16 == 0, hidden <= 1024");
        if (pb->max_labels < 1 || pb->max_labels > kJsMaxU)
          return fail(LT_EUNSUPPORTED, "lt_joint_string_rows: needs 1 <= max_labels <= 4095");
        return LT_OK;
      }))
    return rc;
  const long long R = g->vocab_size + 1, H = jp->hidden, U1 = pb->max_labels + 1;
  const long long B = pb->batch;
  if (B * ((U1 + 31) / 32) * std::max(1, pb->max_frames) > 0x7fffffffLL)
    return fail(LT_EUNSUPPORTED, "lt_joint_string_rows: 2^31 workgroups or more");
  const bool sp = jp->precision == LT_JOINT_SPLIT;
  auto up16 = [](long long x) { return (x + 15) & ~15LL; };
  auto up256 = [](long long x) { return (x + 255) & ~255LL; };
  const long long wob = up16((sp ? 4LL : 2LL) * ((R * (H + 8) + 7) & ~7LL));
  const long long ctxb = 4LL * 32 * (H + 4), rowb = 4 * H;
  // the 32 context rows in LDS while at least 4 waves' frame rows fit beside
  // them, as many waves as fit up to 16; else 8 (or 4) waves that read their
  // context rows from the workspace
  long long nw = (kJsLds - wob - ctxb) / rowb;
  pl->stage_ctx = nw >= 4 ? 1 : 0;
  if (pl->stage_ctx) {
    nw = std::min(nw, 16LL);
  } else {
    nw = (kJsLds - wob) / rowb >= 8 ? 8 : 4;
    if (wob + nw * rowb > kJsLds)
      return fail(LT_EUNSUPPORTED, "lt_joint_string_rows: the output projection and the frame "
                                   "rows exceed the CU's 160 KB of LDS");
  }
  pl->nw = (int)nw;
  pl->o_ctx = (int)wob;
  pl->o_crow = (int)(wob + (pl->stage_ctx ? ctxb : 0));
  pl->lds = (int)(pl->o_crow + nw * rowb);
  pl->stage_tab = stage_table(g, kJsStageTab) ? 1 : 0;
  pl->hdr_bytes = (size_t)up256(8 * B);
  pl->st_bytes = (size_t)up256(4 * B * U1);
  pl->row_bytes = (size_t)(4 * B * U1 * H);
  return LT_OK;
}

template <bool OBF16, bool SP>
auto jstr_pick(bool two) {
  return two ? jstr_rows_kernel<OBF16, true, SP> : jstr_rows_kernel<OBF16, false, SP>;
}

}  // namespace

extern "C" {

int lt_joint_string_rows_workspace_bytes(const lt_graph* g, const lt_table_problem* pb,
                                         const lt_joint_params* jp, size_t* bytes) {
  JsPlan pl;
  if (int rc = jstr_plan(g, pb, jp, &pl)) return rc;
  if (bytes) *bytes = pl.hdr_bytes + pl.st_bytes + pl.row_bytes;
  return LT_OK;
}

int lt_joint_string_rows(const lt_graph* g, const lt_table_problem* pb, const lt_joint_params* jp,
                         const int32_t* num_frames, const int32_t* labels,
                         const int32_t* num_labels, void* Ws, int32_t* states, void* workspace,
                         size_t workspace_bytes, void* stream) {
  JsPlan pl;
  if (int rc = jstr_plan(g, pb, jp, &pl)) return rc;
  if (pb->batch == 0) return LT_OK;
  if (!num_frames || !labels || !jp->ctx_proj || !jp->out_weight || !jp->out_bias ||
      ((!jp->frame_proj || !Ws) && pb->max_frames > 0))
    return fail(LT_EINVAL, "lt_joint_string_rows: null pointer");
  if (!workspace || workspace_bytes < pl.hdr_bytes + pl.st_bytes + pl.row_bytes)
    return fail(LT_EINVAL, "lt_joint_string_rows: workspace too small");
  const bool bf = pb->weight_dtype == LT_DTYPE_BF16;
  if (((uintptr_t)jp->ctx_proj & 15) || ((uintptr_t)jp->frame_proj & 15) ||
      ((uintptr_t)workspace & 15) || ((uintptr_t)jp->out_weight & 3) ||
      ((uintptr_t)jp->out_bias & 3) || ((uintptr_t)num_frames & 3) || ((uintptr_t)labels & 3) ||
      ((uintptr_t)num_labels & 3) || ((uintptr_t)states & 3) || ((uintptr_t)Ws & (bf ? 1 : 3)))
    return fail(LT_EINVAL, "lt_joint_string_rows: misaligned pointer");
  char* ws = (char*)workspace;
  JsArgs a;
  memset(&a, 0, sizeof(a));
  a.table = g->next_state;
  a.labels = labels;
  a.nfr = num_frames;
  a.pc = jp->ctx_proj;
  a.pf = jp->frame_proj;
  a.wo = jp->out_weight;
  a.bias = jp->out_bias;
  a.Ws = Ws;
  a.states = states;
  a.hdr = (int*)ws;
  a.st = (int*)(ws + pl.hdr_bytes);
  a.rows = (float*)(ws + pl.hdr_bytes + pl.st_bytes);
  a.B = pb->batch;
  a.T = pb->max_frames;
  a.U = pb->max_labels;
  a.C = g->num_states;
  a.V = g->vocab_size;
  a.R = g->vocab_size + 1;
  a.H = jp->hidden;
  a.NT = (a.U + 1 + 31) / 32;
  a.nw = pl.nw;
  a.stage_ctx = pl.stage_ctx;
  a.stage_tab = pl.stage_tab;
  a.o_ctx = pl.o_ctx;
  a.o_crow = pl.o_crow;
  // frame slices: about two workgroups a CU over the whole grid, a slice no
  // shorter than a frame per wave
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess)
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  const long long pairs = (long long)a.B * a.NT;
  long long S = std::max<long long>(1, (2LL * cus + pairs - 1) / pairs);
  S = std::min<long long>(S, std::max(1, (a.T + pl.nw - 1) / pl.nw));
  a.FL = std::max(1, (int)((a.T + S - 1) / S));
  a.S = std::max(1, (a.T + a.FL - 1) / a.FL);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = launch(jstr_walk_kernel, dim3((unsigned)a.B), dim3(kJsWalkThreads),
                      (int)stage_table(g, kJsStageTab), st, a, "joint string rows",
                      " walk kernel launch"))
    return rc;
  if (a.T == 0) return LT_OK;
  const bool sp = jp->precision == LT_JOINT_SPLIT, two = a.R > 32;
  auto k = sp ? (bf ? jstr_pick<true, true>(two) : jstr_pick<false, true>(two))
              : (bf ? jstr_pick<true, false>(two) : jstr_pick<false, false>(two));
  return launch(k, dim3((unsigned)(pairs * a.S)), dim3(64 * pl.nw), pl.lds, st, a,
                "joint string rows");
}

}  // extern "C"
