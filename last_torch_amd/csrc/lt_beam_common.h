// lt_beam_common.h -- the part of the prefix beam search (include/lt_beam.h)
// that does not depend on where the arc weights come from: the slot state, the
// prefix hash, one frame of the search (merge, select, the new beam, the trace
// row) and the outputs with the in-launch backtrace. lt_beam.hip searches W
// from memory (a slot's weight row is its context state's row of a staged
// frame); lt_beam_joint.hip forms the beam's rows on the matrix cores (a
// slot's weight row is the row of its own index in a [64][R] LDS tile).
#ifndef LT_BEAM_COMMON_H_
#define LT_BEAM_COMMON_H_

#include "lt_string_common.h"

namespace {

struct BArgs {
  const unsigned char* W;
  const int* nfr;
  const int* table;   // [C, V] next state of (p, y)
  long long* labels;  // [B, K, T]
  int* nlab;          // [B, K]
  float* scores;      // [B, K]
  int* trace;         // [B, T, K] (the caller's, or the workspace)
  float* step;        // [B, T, K] or null
  int pad_trace;      // the padding frames of `trace` are an output
  int B, T, C, V, R, K;
  int L;          // frames per ring slice (0: no ring)
  int capW;       // 16-byte chunks of a slice's image
  int MW;         // 32-bit words of a slot's removed-label mask
  int stage_tab;  // the next-state table is staged in LDS
};

constexpr int kBeamMaxK = 64;
constexpr int kBeamMaxV = 1023;

LT_DEVINL unsigned long long readlane64(unsigned long long v, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}
LT_DEVINL unsigned long long shfl64(unsigned long long v, int l) {
  const unsigned lo = (unsigned)__shfl((int)(unsigned)v, l);
  const unsigned hi = (unsigned)__shfl((int)(unsigned)(v >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}

// the hash of prefix + y (include/lt_beam.h)
LT_DEVINL unsigned long long mix(unsigned long long h, int y) {
  unsigned long long z = h ^ ((unsigned long long)y * 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// a candidate: one fp32 add, NaN counts as -inf
LT_DEVINL float cand(float s, float w) {
  const float v = s + w;
  return v == v ? v : -kInf;
}

// The slot state of the searching wave: lane r is slot r.
struct Slot {
  float s;                    // score; -inf: dead
  int c, n, y;                // context state, length, last label
  unsigned long long h, ph;   // hash of the prefix, of its parent
};

// Lane l's first candidate k = l as (slot, label) = (l / R, l % R), and the
// step of k += 64.
struct LaneDeal {
  int i0, y0, di, dy;
};

// One frame of the search (wave 0, all 64 lanes active). wf: the frame's
// weight rows of R elements -- W [C, R], a slot reads its context state's row
// (SLOTROW false), or a [64, R] tile formed for this beam, slot i reads row i
// (SLOTROW true; the merge then finds the parent's row by the parent's slot);
// mrows: the slots' mask rows in LDS, MW words each (bit y: candidate
// (slot, y) is removed or taken); sbuf: the slots' (score, state, blank
// candidate) in LDS; tbl: the table.
template <int MODE, bool BF16, bool SLOTROW>
LT_DEVINL void beam_frame(Slot& q, int& nlive, const unsigned char* wf, unsigned* mrows,
                          float4* sbuf, const int* tbl, const BArgs& a, const LaneDeal& ld,
                          int lane, long long tro) {
  constexpr int ES = BF16 ? 2 : 4;
  const int R = a.R, MW = a.MW;
  unsigned* mask = mrows + lane * MW;  // this slot's row
  const bool live = lane < nlive;
  const unsigned char* row = wf + (long long)(SLOTROW ? lane : q.c) * R * ES;
  float cb = live ? cand(q.s, ldw<BF16>(row, 0)) : -kInf;
  for (int w = 0; w < MW; ++w) mask[w] = 0;
  // ---- merge
  bool hasp = false;
  float ps = 0.f;
  int pc = 0;  // the parent's weight row
  for (int j = 0; j < nlive; ++j) {
    const unsigned long long hj = readlane64(q.h, j), phj = readlane64(q.ph, j);
    const int nj = __builtin_amdgcn_readlane(q.n, j), yj = __builtin_amdgcn_readlane(q.y, j);
    const int cj = __builtin_amdgcn_readlane(q.c, j);
    const float sj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(q.s), j));
    if (live && !hasp && q.n >= 1 && hj == q.ph && nj == q.n - 1) {  // j is my parent
      hasp = true;
      ps = sj;
      pc = SLOTROW ? j : cj;
    }
    if (live && nj >= 1 && phj == q.h && nj - 1 == q.n)  // j is my child
      mask[yj >> 5] |= 1u << (yj & 31);
  }
  if (hasp) {
    const float e = cand(ps, ldw<BF16>(wf + (long long)pc * R * ES, q.y));
    cb = MODE == M_LOG ? log_plus(cb, e) : (cb >= e ? cb : e);
    if (!(cb == cb)) cb = -kInf;
  }
  // ---- select: the candidates dealt round-robin to the 64 lanes, each
  // lane's four best in registers, then K rounds over the wave
  sbuf[lane] = make_float4(q.s, __int_as_float(q.c), cb, 0.f);
  float s0, s1, s2, s3;  // this lane's best candidates not yet taken, best first
  int p0, p1, p2, p3;    // as (slot << 16) | label: ordered as k = slot*R + label
  int nfin, wins;        // finite candidates the last scan saw; taken since
  auto insert = [&](float v, int p) {
    if (!(v > -kInf)) return;  // -inf and NaN are no candidates
    ++nfin;
    // after every element >= v: equal scores keep the scan's order, ascending k
    // (g0 implies g1 implies g2 implies g3, so the displaced one moves down)
    const bool g0 = v > s0, g1 = v > s1, g2 = v > s2, g3 = v > s3;
    float cs = v, ts;
    int cp = p, tp;
#define LT_BEAM_STAGE(G, S, P) \
  ts = S; tp = P;              \
  S = G ? cs : ts; P = G ? cp : tp; \
  cs = G ? ts : cs; cp = G ? tp : cp;
    LT_BEAM_STAGE(g0, s0, p0)
    LT_BEAM_STAGE(g1, s1, p1)
    LT_BEAM_STAGE(g2, s2, p2)
    LT_BEAM_STAGE(g3, s3, p3)
#undef LT_BEAM_STAGE
  };
  const int N = nlive * R;  // candidates k = slot*R + label; lane l has k = l, l + 64, ...
  auto scan = [&]() {
    s0 = s1 = s2 = s3 = -kInf;
    p0 = p1 = p2 = p3 = 0;
    nfin = wins = 0;
    int i = ld.i0, y = ld.y0;
    for (int k = lane; k < N;) {  // four candidates in flight
      float v[4];
      int p[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool ok = k < N;
        const int ii = ok ? i : 0, yy = ok ? y : 0;
        const float4 sl = sbuf[ii];  // (score, state, merged blank candidate)
        const unsigned m = mrows[ii * MW + (yy >> 5)];
        const float w = ldw<BF16>(wf + (long long)(SLOTROW ? ii : __float_as_int(sl.y)) * R * ES, yy);
        const bool gone = (m >> (yy & 31)) & 1;  // removed by the merge, or taken
        v[u] = ok && !gone ? (yy == 0 ? sl.z : sl.x + w) : -kInf;
        p[u] = (ii << 16) | yy;
        k += 64;
        i += ld.di;
        y += ld.dy;
        if (y >= R) {
          y -= R;
          ++i;
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) insert(v[u], p[u]);
    }
  };
  scan();
  float ns = -kInf;
  int np = 0, nnew = 0;
  for (int r = 0; r < a.K; ++r) {
    const float top = wave_max(s0);
    if (!(top > -kInf)) break;  // no candidate left
    unsigned long long m = __ballot(s0 == top);
    int src = __ffsll((long long)m) - 1;
    int pw = __builtin_amdgcn_readlane(p0, src);
    for (m &= m - 1; m; m &= m - 1) {  // equal scores (rare): the smallest k
      const int l = __ffsll((long long)m) - 1;
      const int pl = __builtin_amdgcn_readlane(p0, l);
      if (pl < pw) {
        pw = pl;
        src = l;
      }
    }
    if (lane == r) {
      ns = top;
      np = pw;
    }
    if (lane == src) {
      mrows[(pw >> 16) * MW + ((pw & 0xffff) >> 5)] |= 1u << (pw & 31);  // taken
      s0 = s1; p0 = p1;
      s1 = s2; p1 = p2;
      s2 = s3; p2 = p3;
      s3 = -kInf; p3 = 0;
      ++wins;
      // the four are used up and the lane holds more: the taken ones are in
      // the masks, scan again
      if (!(s0 > -kInf) && wins < nfin) scan();
    }
    nnew = r + 1;
  }
  const int nsrc = np >> 16, nyw = np & 0xffff;
  // ---- the new beam, from the old one through ds_bpermute
  const unsigned long long sh = shfl64(q.h, nsrc), sph = shfl64(q.ph, nsrc);
  const int sn = __shfl(q.n, nsrc), sc = __shfl(q.c, nsrc), sy = __shfl(q.y, nsrc);
  const bool kept = lane < nnew;
  Slot z = {-kInf, 0, 0, 0, 0ull, 0ull};
  if (kept) {
    z.s = ns;
    if (nyw == 0) {
      z.c = sc; z.n = sn; z.y = sy; z.h = sh; z.ph = sph;
    } else {
      z.c = tbl[(long long)sc * a.V + nyw - 1];
      z.n = sn + 1;
      z.y = nyw;
      z.h = mix(sh, nyw);
      z.ph = sh;
    }
  }
  q = z;
  nlive = nnew;
  if (lane < a.K) {
    a.trace[tro + lane] = kept ? (nsrc << 16) | nyw : -1;
    if (a.step) a.step[tro + lane] = kept ? ns : -kInf;
  }
}

// After the last live frame (wave 0, all lanes): scores, lengths, the zeros
// behind each label sequence, then the label sequences read back from the
// trace rows of utterance b (at tr0), which other lanes of this wave stored.
LT_DEVINL void beam_finish(const Slot& q, int nlive, const BArgs& a, int b, int nf, int lane,
                           long long tr0) {
  const int T = a.T, K = a.K;
  if (lane < K) {
    a.scores[(long long)b * K + lane] = q.s;
    a.nlab[(long long)b * K + lane] = q.n;
  }
  long long* out = a.labels + (long long)b * K * T;
  for (int k = 0; k < K; ++k) {
    const int nk = __builtin_amdgcn_readlane(q.n, k);
    for (int p = nk + lane; p < T; p += 64) out[(long long)k * T + p] = 0;
  }
  __threadfence();
  if (lane < nlive) {
    int cur = lane, pos = q.n;
    for (int t = nf - 1; t >= 0 && pos > 0; --t) {
      const int e = a.trace[tr0 + (long long)t * K + cur];
      if (e < 0) break;
      const int y = e & 0xffff;
      if (y) out[(long long)lane * T + --pos] = y;
      cur = e >> 16;
    }
  }
}

}  // namespace

#endif  // LT_BEAM_COMMON_H_
