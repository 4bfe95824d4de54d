// Linear-chain CRF on top of the BiLSTM tagger (engine/tagger.py): the negative log-likelihood with all of its
// gradients in one launch (rk_crf_nll), and Viterbi decoding (rk_crf_viterbi).
//
// Model: a path y of a sentence of n tokens scores start[y_0] + sum_t e_t(y_t) + sum_{t>=1} trans[y_{t-1}][y_t] +
// end[y_{n-1}]; e_t is the output layer's logit row of token (t, b), row t * B + b, leading dimension NTP = NT
// rounded up to 4, and trans / start / end are padded to NTP the same way.  loss = sum_b (logZ_b - score_b(gold)) * inv.
//
// Work split: one 64-lane wave per sentence, lane j owns tag j (NT <= 64), four sentences per block.  The recursion
// is serial in t and the B sentences are all the parallelism there is, so what counts is the length of one step:
//   * lane j holds column j of exp(trans - colmax_j) in registers for the whole sentence (the column maximum moves
//     into the emission term, so every entry is <= 1); the backward walk adds row j of the same matrix;
//   * the value of lane i reaches the other lanes by v_readlane in a loop over i unrolled at compile time (the
//     kernels are instantiated for 16 / 32 / 48 / 64 tags) — no LDS, no dynamic register index, no scratch;
//   * scaled exp domain: u_t(j) = (sum_i u_{t-1}(i) E[i][j]) * exp(x_t(j) - m_t) / c_{t-1} with m_t = max_j x_t(j)
//     and c_{t-1} = sum_i u_{t-1}(i).  c_{t-1} is summed in the same unrolled loop from the broadcast values, so the
//     renormalisation costs no cross-lane reduction on the serial path; m_t depends on the emissions alone and is
//     prepared one step ahead.  One exp and one log per lane and step; log Z = sum_t (m_t + log c_{t-1}) + the
//     closing term with end[];
//   * emissions are fetched two steps ahead of the step that prepares them (three ahead of their use);
//   * the forward walk saves u_t [L][B][NTP] and the per-step scales (m_t, 1 / c_{t-1}) in the workspace; the same
//     wave then walks t = n-1 .. 0 with b_t scaled so that u_t(j) * b_t(j) is the marginal of tag j — the saved
//     scales make that exact with no reduction per step — and writes one coalesced d(logits) row per step
//     ((marginal - gold) * inv; zeros for t >= n and for the pad columns);
//   * lane j accumulates column j of the transition gradient in registers, sum_t xi_t(i, j) - [gold_{t-1} = i and
//     gold_t = j], the gold term as a compare of the unrolled i against the wave-uniform previous tag.
// Gradients are deterministic: every wave writes its partial transition / start / end gradients to the workspace
// and crf_fold_kernel adds them in sentence order and scales by inv.  Only the scalar loss uses a float atomic, as
// the softmax cross-entropy kernel does.
//
// Viterbi has the same mapping with the raw transition column: max-plus in the log domain (no exp), strict '>' over
// ascending i so ties go to the lowest tag, one-byte backpointers in LDS while a block's 4 * L * 64 bytes fit into
// 64 KiB and in the workspace beyond that, then a backtrace by the same wave.
//
// Why no matrix instructions: per step the batch-level product is [B, NT] x [NT, NT] with NT <= 64 and B <= 128, it
// sits on the serial dependency, and every row carries a scale of its own.  An MFMA would add its issue and
// accumulator-read latency to the one thing that bounds these kernels; 64 readlane + FMA pairs per step are shorter.
#include "common.h"

namespace {

constexpr int CRF_WAVES = 4;   // sentences per block

RK_DEV float lane_bcast(float v, int i) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), i));
}

RK_DEV int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// workspace of rk_crf_nll, in floats: u [L][B][NTP] | scales [L][B][2] | partials [B][NTP * NTP + 2 * NTP]
struct CrfWs {
  long long u, scales, part, total;
};
static CrfWs crf_ws(int L, int B, int NTP) {
  CrfWs w;
  w.u = 0;
  w.scales = (long long)L * B * NTP;
  w.part = w.scales + (long long)L * B * 2;
  w.total = w.part + (long long)B * (NTP * NTP + 2 * NTP);
  return w;
}

// what the backward walk reads per step: emission, saved scales, saved u, gold tag
struct CrfRec {
  float e, m, k, u;
  int g;
};

template <int NI>
__global__ __launch_bounds__(256) void crf_nll_kernel(const float* __restrict__ emis, const float* __restrict__ trans,
                                                      const float* __restrict__ start, const float* __restrict__ end,
                                                      const int* __restrict__ labels, const int* __restrict__ lens,
                                                      int L, int B, int NT, int NTP, const float* __restrict__ inv_p,
                                                      float* __restrict__ dlog, float* __restrict__ loss_sum,
                                                      float* ualpha, float* scales, float* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * CRF_WAVES + (threadIdx.x >> 6);
  if (b >= B) return;   // (no block-level barrier in this kernel)
  const bool live = lane < NT, inpad = lane < NTP;
  const int n = clampi(lens[b], 0, L);
  const float inv = inv_p[0];
  const float NEG = -INFINITY;
  const long long rs = (long long)B * NTP;                 // floats between the rows of t and t + 1
  const long long col = (long long)b * NTP + lane;
  const float* eb = emis + col;
  float* ub = ualpha + col;
  float* db = dlog + col;
  float* sc = scales + (long long)b * 2;                   // + t * B * 2
  float* pt = part + (long long)b * (NTP * NTP + 2 * NTP);

  if (inpad)
    for (int t = n; t < L; ++t) db[t * rs] = 0.f;
  if (n == 0) {
    if (inpad) {
      for (int i = 0; i < NTP + 2; ++i) pt[i * NTP + lane] = 0.f;
    }
    return;
  }

  // column j of the transitions: raw -> exp(. - colmax); rows / lanes >= NT are zero
  float acol[NI];
  float cmax = NEG;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    acol[i] = (live && i < NT) ? trans[i * NTP + lane] : NEG;
    cmax = fmaxf(cmax, acol[i]);
  }
  if (!live) cmax = 0.f;
#pragma unroll
  for (int i = 0; i < NI; ++i) acol[i] = expf(acol[i] - cmax);

  // the gold path's score, each lane the terms of its own tag: no serial dependency, and it warms the caches
  float gs = 0.f;
  {
    int gp = 0;
    for (int t = 0; t < n; ++t) {
      const int g = clampi(labels[(long long)t * B + b], 0, NT - 1);
      if (live) {
        const float add = eb[t * rs] + (t == 0 ? start[lane] : trans[gp * NTP + lane]);
        gs += lane == g ? add : 0.f;
      }
      gp = g;
    }
    if (live) gs += lane == gp ? end[lane] : 0.f;
  }

  // ---- forward: u_t, log-scale acc
  const float x0 = live ? eb[0] + start[lane] : NEG;
  float acc = wave_max(x0);
  float u = expf(x0 - acc);
  if (inpad) ub[0] = u;
  {
    float e1 = (1 < n && live) ? eb[rs] : 0.f;             // raw emissions of t + 1 (here t = 0)
    float e2 = (2 < n && live) ? eb[2 * rs] : 0.f;         // and t + 2
    float x = live ? e1 + cmax : NEG;
    float m1 = wave_max(x), q1 = expf(x - m1);             // prepared for step 1
    for (int t = 1; t < n; ++t) {
      const float e3 = (t + 2 < n && live) ? eb[(t + 2) * rs] : 0.f;
      x = live ? e2 + cmax : NEG;                          // prepare step t + 1
      const float m2 = wave_max(x), q2 = expf(x - m2);
      float s0 = 0.f, s1 = 0.f, c0 = 0.f, c1 = 0.f;
#pragma unroll
      for (int i = 0; i < NI; i += 2) {
        const float a0 = lane_bcast(u, i), a1 = lane_bcast(u, i + 1);
        s0 = fmaf(a0, acol[i], s0);
        s1 = fmaf(a1, acol[i + 1], s1);
        c0 += a0;
        c1 += a1;
      }
      const float c = c0 + c1, k = 1.0f / c;
      u = (s0 + s1) * (q1 * k);
      acc += m1 + logf(c);
      if (inpad) ub[t * rs] = u;
      sc[(long long)t * B * 2] = m1;                       // every lane stores (and later reads) the same two words
      sc[(long long)t * B * 2 + 1] = k;
      m1 = m2, q1 = q2, e2 = e3;
    }
  }

  // ---- closing term, loss, b_{n-1}
  const float y = live ? end[lane] : NEG;
  const float me = wave_max(y), ye = expf(y - me);
  const float ce = wave_sum(u * ye);
  gs = wave_sum(gs);
  if (lane == 0 && loss_sum) atomicAdd(loss_sum, (acc + me + logf(ce) - gs) * inv);
  float bt = ye / ce;

  // ---- backward: row j of the same matrix, the transition gradient's column in registers
  float arow[NI], gacc[NI];
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const float cj = lane_bcast(cmax, j);
    arow[j] = (live && j < NT) ? expf(trans[lane * NTP + j] - cj) : 0.f;
    gacc[j] = 0.f;
  }
  auto load = [&](int t) {
    CrfRec r = {0.f, 0.f, 0.f, 0.f, 0};
    if (t >= 0) {
      r.e = live ? eb[t * rs] : 0.f;
      r.u = inpad ? ub[t * rs] : 0.f;
      r.g = clampi(labels[(long long)t * B + b], 0, NT - 1);
      if (t >= 1) r.m = sc[(long long)t * B * 2], r.k = sc[(long long)t * B * 2 + 1];
    }
    return r;
  };
  auto factor = [&](const CrfRec& r) { return expf((live ? r.e + cmax : NEG) - r.m) * r.k; };
  CrfRec r0 = load(n - 1), r1 = load(n - 2), r2 = load(n - 3);
  float rf0 = factor(r0);
  float g_start = 0.f, g_end = 0.f;
  for (int t = n - 1; t >= 0; --t) {
    const CrfRec r3 = load(t - 3);
    const float rf1 = factor(r1);                          // of step t - 1, off the serial path
    const float gj = (live && lane == r0.g) ? 1.f : 0.f;
    const float d = r0.u * bt - gj;
    if (inpad) db[t * rs] = d * inv;
    if (t == n - 1) g_end = d;
    if (t == 0) g_start = d;
    if (t >= 1) {
      const float w = rf0 * bt;
      const int gprev = __builtin_amdgcn_readfirstlane(r1.g);
      float n0 = 0.f, n1 = 0.f;
#pragma unroll
      for (int i = 0; i < NI; i += 2) {
        n0 = fmaf(arow[i], lane_bcast(w, i), n0);
        n1 = fmaf(arow[i + 1], lane_bcast(w, i + 1), n1);
      }
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        gacc[i] = fmaf(lane_bcast(r1.u, i), acol[i] * w, gacc[i]);
        gacc[i] -= i == gprev ? gj : 0.f;
      }
      bt = n0 + n1;
    }
    r0 = r1, r1 = r2, r2 = r3, rf0 = rf1;
  }
  if (inpad) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
      if (i < NTP) pt[i * NTP + lane] = gacc[i];
    pt[NTP * NTP + lane] = g_start;
    pt[NTP * NTP + NTP + lane] = g_end;
  }
}

// g_trans | g_start | g_end = inv * sum over the sentences' partials, in sentence order
__global__ __launch_bounds__(256) void crf_fold_kernel(const float* __restrict__ part, int B, int NTP,
                                                       const float* __restrict__ inv_p, float* __restrict__ g_trans,
                                                       float* __restrict__ g_start, float* __restrict__ g_end) {
  const int total = NTP * NTP + 2 * NTP;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  float s = 0.f;
  for (int b = 0; b < B; ++b) s += part[(long long)b * total + i];
  s *= inv_p[0];
  if (i < NTP * NTP) g_trans[i] = s;
  else if (i < NTP * NTP + NTP) g_start[i - NTP * NTP] = s;
  else g_end[i - NTP * NTP - NTP] = s;
}

template <int NI>
__global__ __launch_bounds__(256) void crf_viterbi_kernel(const float* __restrict__ emis,
                                                          const float* __restrict__ trans,
                                                          const float* __restrict__ start,
                                                          const float* __restrict__ end, const int* __restrict__ lens,
                                                          int L, int B, int NT, int NTP, int* __restrict__ tags,
                                                          unsigned char* bp_ws) {
  extern __shared__ unsigned char bp_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * CRF_WAVES + wave;
  const bool live = lane < NT;
  const int n = b < B ? clampi(lens[b], 0, L) : 0;
  const float NEG = -INFINITY;
  // backpointers [t][lane] of this wave's sentence (row 0 unused)
  unsigned char* bp = bp_ws ? bp_ws + (long long)(b < B ? b : 0) * L * 64 : bp_lds + (long long)wave * L * 64;
  int best_tag = 0;
  if (n > 0) {
    float tcol[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) tcol[i] = (live && i < NT) ? trans[i * NTP + lane] : NEG;
    const long long rs = (long long)B * NTP;
    const float* eb = emis + (long long)b * NTP + lane;
    float d = live ? eb[0] + start[lane] : NEG;
    float e1 = (1 < n && live) ? eb[rs] : 0.f, e2 = (2 < n && live) ? eb[2 * rs] : 0.f;
    for (int t = 1; t < n; ++t) {
      const float e3 = (t + 2 < n && live) ? eb[(t + 2) * rs] : 0.f;
      float best = lane_bcast(d, 0) + tcol[0];
      int arg = 0;
#pragma unroll
      for (int i = 1; i < NI; ++i) {
        const float v = lane_bcast(d, i) + tcol[i];
        if (v > best) best = v, arg = i;                   // strict: ties keep the lowest predecessor
      }
      d = live ? best + e1 : NEG;
      bp[t * 64 + lane] = (unsigned char)arg;
      e1 = e2, e2 = e3;
    }
    float f = live ? d + end[lane] : NEG;
    best_tag = lane;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float of = __shfl_xor(f, o, 64);
      const int ot = __shfl_xor(best_tag, o, 64);
      if (of > f || (of == f && ot < best_tag)) f = of, best_tag = ot;
    }
  }
  __syncthreads();   // the wave's backpointer stores are visible to all of its lanes
  if (b >= B) return;
  int tag = best_tag;
  for (int t = n - 1; t >= 0; --t) {
    if (lane == 0) tags[(long long)b * L + t] = tag;
    if (t > 0) tag = bp[t * 64 + tag];
  }
  for (int t = n + lane; t < L; t += 64) tags[(long long)b * L + t] = -1;
}

inline int crf_ntp(int NT) { return (NT + 3) & ~3; }

}  // namespace

#define RK_CRF_DISPATCH(NT, KERNEL, ...)                                   \
  do {                                                                     \
    if ((NT) <= 16) hipLaunchKernelGGL(KERNEL<16>, __VA_ARGS__);           \
    else if ((NT) <= 32) hipLaunchKernelGGL(KERNEL<32>, __VA_ARGS__);      \
    else if ((NT) <= 48) hipLaunchKernelGGL(KERNEL<48>, __VA_ARGS__);      \
    else hipLaunchKernelGGL(KERNEL<64>, __VA_ARGS__);                      \
  } while (0)

// bytes of the workspace that rk_crf_nll and rk_crf_viterbi take for a [L, B] batch of NT tags (0: bad arguments)
extern "C" long long rk_crf_ws_bytes(int L, int B, int NT) {
  if (L <= 0 || B <= 0 || NT < 1 || NT > 64) return 0;
  const long long nll = crf_ws(L, B, crf_ntp(NT)).total * 4, vit = (long long)L * B * 64;
  return nll > vit ? nll : vit;
}

// loss and gradients of one batch.  emis / dlogits [L * B][NTP] time-major, trans [NTP][NTP], start / end [NTP],
// labels [L * B] time-major (read for t < lens[b] only), inv a device float; loss_sum[0] += loss (nullable).
extern "C" int rk_crf_nll(const float* emis, const float* trans, const float* start, const float* end,
                          const int* labels, const int* lens, int L, int B, int NT, const float* inv, float* dlogits,
                          float* g_trans, float* g_start, float* g_end, float* loss_sum, void* ws, void* stream) {
  if (NT < 1 || NT > 64 || L < 0 || B < 0) return RK_EBADARG;
  if (L == 0 || B == 0) return RK_OK;
  if (!emis || !trans || !start || !end || !labels || !lens || !inv || !dlogits || !g_trans || !g_start || !g_end || !ws)
    return RK_EBADARG;
  const int NTP = crf_ntp(NT);
  const CrfWs w = crf_ws(L, B, NTP);
  float* f = (float*)ws;
  RK_CRF_DISPATCH(NT, crf_nll_kernel, dim3(rk_cdiv(B, CRF_WAVES)), dim3(256), 0, (hipStream_t)stream, emis, trans,
                  start, end, labels, lens, L, B, NT, NTP, inv, dlogits, loss_sum, f + w.u, f + w.scales, f + w.part);
  RK_LAUNCH_CHECK();
  hipLaunchKernelGGL(crf_fold_kernel, dim3(rk_cdiv(NTP * NTP + 2 * NTP, 256)), dim3(256), 0, (hipStream_t)stream,
                     f + w.part, B, NTP, inv, g_trans, g_start, g_end);
  RK_LAUNCH_CHECK();
  return RK_OK;
}

// best path of every sentence: tags [B][L] int32, -1 for t >= lens[b]
extern "C" int rk_crf_viterbi(const float* emis, const float* trans, const float* start, const float* end,
                              const int* lens, int L, int B, int NT, int* tags, void* ws, void* stream) {
  if (NT < 1 || NT > 64 || L < 0 || B < 0) return RK_EBADARG;
  if (L == 0 || B == 0) return RK_OK;
  if (!emis || !trans || !start || !end || !lens || !tags) return RK_EBADARG;
  const long long lds = (long long)CRF_WAVES * L * 64;
  const bool in_lds = lds <= 65536;
  if (!in_lds && !ws) return RK_EBADARG;
  RK_CRF_DISPATCH(NT, crf_viterbi_kernel, dim3(rk_cdiv(B, CRF_WAVES)), dim3(256), in_lds ? (unsigned)lds : 0u,
                  (hipStream_t)stream, emis, trans, start, end, lens, L, B, NT, crf_ntp(NT), tags,
                  in_lds ? nullptr : (unsigned char*)ws);
  RK_LAUNCH_CHECK();
  return RK_OK;
}
