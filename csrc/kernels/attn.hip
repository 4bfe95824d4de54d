// Fused masked multi-head self-attention for gfx950, fp32 (PyBiLstmAttn / PyBiLstmAttnCrf through engine/tagger.py):
// ctx = softmax(scale Q K^T + key mask) V per sentence and head, and its gradient, without the score matrix ever
// leaving registers.  Sentences of 1..250 tokens, head dims 8..32 (zero-padded to DP in {16, 32}), up to 8 heads.
//
//   rows are time-major, row = t * B + b;  qkv [n][3][NH][DP] (one S.linear's output);  ctx, dctx [n][NH][DP];
//   lse [n][NH];  lens int32 [B] (clamped to 0..L);  scale = 1 / sqrt(true head dim)
//   s[i][j] = scale q_i . k_j for j < lens[b]   p = softmax_j(s)   ctx_i = sum_j p[i][j] v_j   lse_i = log sum_j exp(s[i][j])
//   query rows i >= lens[b] get ctx = 0, lse = 0, and dqkv = 0 in all three parts; every launch writes every element.
//   The padded d columns (true head dim .. DP) of ctx and dqkv are exact zeros because those columns of qkv and dctx
//   are: the kernels rely on the arena's zero-padding rule for them and do not mask columns themselves.
//
// Work split.  An item is (sentence b, head h, group of 64 rows); a workgroup of 4 waves takes items in a stride loop
// over a capped grid, wave w owning the 16-row tile 4 g + w.  The other side's rows (keys for the forward) come in
// chunks of 64 through LDS, staged once for the four waves (float4 global loads, each row a contiguous DP-float
// segment; LDS row stride DP + 1); rows >= lens[b] are staged as zeros and never read from memory, and the loop ends
// at ceil(lens[b] / 16) tiles.  All trip counts that reach a barrier depend on (b, h, g) only.
//
// Forward (attn_fwd_kernel<DP>).  Transposed scores S^T = K Q^T on DP/4 v_mfma_f32_16x16x4_f32: A = the key tile from
// LDS, B = the wave's Q fragment, resident in registers for the whole key loop.  In the D layout lane (c = lane & 15,
// g = lane >> 4) holds keys 4 g .. 4 g + 3 of query c, so a query's max and sum are 4 in-lane values and two
// cross-lane steps (xor 16, 32), and the online-softmax rescale is one factor a lane.  P^T in that layout is already
// the B operand of O^T[d][query] += V^T[d][key] P^T[key][query]: MFMA r takes each lane's register r, and its A
// operand reads V at key 4 g + r (a sum over keys does not care about their order), so P takes no LDS round trip
// and no shuffle.  Keys past lens[b] in the last tile are set to -inf by row of S^T.  A lane ends with 4 consecutive
// d of one query: ctx leaves as float4 stores.  The k index of the score MFMAs is permuted the same way (step s,
// group g -> d = 16 (s >> 2) + 4 g + (s & 3)) so that the register fragments are float4 loads.  The running max and
// lse stay in natural units (scores times scale, as a plain softmax has them) and log2(e) multiplies the exp2
// argument: folding it into scale would round every score once more and lse with it.
//
// Backward (attn_bwd_kernel<DP>, one launch, grid (G, 2)), P recomputed from lse, bit-reproducible, no atomics: each
// role is the sole owner of what it writes.
//   role 0, dQ: wave per query tile, Q, dO and ctx fragments resident, K and V chunks in LDS:
//     S^T, P^T = exp(S^T - lse),  dP^T = V dO^T,  dS^T = P^T (dP^T - delta),
//     dQ^T += K^T dS^T with dS^T taken from registers as P^T is in the forward.
//   role 1, dK and dV: wave per key tile, K and V fragments resident, Q and dO chunks in LDS (and the chunk's lse),
//     non-transposed S = Q K^T so that a lane holds 4 queries of one key:
//     dV^T += dO^T P,  dP = dO V^T,  dK^T += Q^T dS, B again from registers.
//   delta_i = dctx_i . ctx_i is the diagonal of one more MFMA chain with the operand dO in the place it has in dP
//   (role 0: ctx dO^T beside V dO^T; role 1: dO ctx^T beside dO V^T, the ctx fragment of each query tile read from
//   global memory) and one cross-lane read.  A scalar dot product would do, but then a sentence of one token, where
//   ctx = v and so dP = delta in exact arithmetic, would get rounding noise in dQ and dK where every reference has an
//   exact zero; from the same instruction on the same operands the two are equal bit for bit.
//   The two roles have the same structure, share the LDS arrays and need about the same registers, so one grid with
//   two roles costs neither role occupancy and the second launch is saved.
//
// Deviations from a wave-per-tile grid: the four waves of a workgroup always share (b, h), so K and V always go
// through LDS once per workgroup; a short sentence leaves some of the four waves with only the zero rows to write.
//
// Resource report (-Rpass-analysis=kernel-resource-usage, gfx950): ScratchSize 0 for all 4 kernels.
//   forward  <16> / <32>: 58 / 66 VGPRs + 4 / 8 AGPRs, LDS 8704 / 16896 B, 8 / 6 waves / SIMD
//   backward <16> / <32>: 102 / 106 VGPRs + 20 / 28 AGPRs, LDS 8960 / 17152 B, 4 / 3 waves / SIMD
#include "common.h"

namespace {

constexpr int QC = 64;            // rows of a staged chunk: 4 waves x 16
constexpr int GRID_CAP = 1024;
constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;

// the d that step s of a score MFMA pairs with k index kq
RK_DEV int frag_d(int s, int kq) { return 16 * (s >> 2) + 4 * kq + (s & 3); }

RK_DEV float4 ld4(const float* p, bool live) {
  return live ? *(const float4*)p : float4{0.f, 0.f, 0.f, 0.f};
}

// f[s] = row[frag_d(s, kq)] (zeros when the row is not live)
template <int DP>
RK_DEV void load_frag(const float* __restrict__ row, bool live, int kq, float (&f)[DP / 4]) {
#pragma unroll
  for (int hf = 0; hf < DP / 16; ++hf) {
    const float4 v = ld4(row + 16 * hf + 4 * kq, live);
    f[4 * hf] = v.x; f[4 * hf + 1] = v.y; f[4 * hf + 2] = v.z; f[4 * hf + 3] = v.w;
  }
}

// sh [64][DP + 1] = rows j0 .. j0 + 63 of sentence b from src (row t * B + b starts at src + row * ld); rows >= len
// are zeros and are not read
template <int DP>
RK_DEV void stage(float* sh, const float* __restrict__ src, size_t ld, int j0, int len, int B, int b) {
  constexpr int LD = DP + 1, V4 = DP / 4;
  for (int i = threadIdx.x; i < QC * V4; i += 256) {
    const int r = i / V4, c = (i % V4) * 4, j = j0 + r;
    const bool live = j < len;
    const float4 v = ld4(src + ((size_t)(live ? j : 0) * B + b) * ld + c, live);
    float* d = sh + r * LD + c;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
}

RK_DEV float xor_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
RK_DEV float xor_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// a * b rounded on its own: no contraction with an add that follows it
RK_DEV float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// v * f for a live row, zeros by a select (not a product, which would pass a NaN or inf on) for any other
RK_DEV void store4(float* p, f32x4 v, float f, bool live) {
  *(float4*)p = live ? float4{v[0] * f, v[1] * f, v[2] * f, v[3] * f} : float4{0.f, 0.f, 0.f, 0.f};
}

template <int DP>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const float* __restrict__ qkv, const int* __restrict__ lens,
                                                       int L, int B, int NH, float scale, float* __restrict__ ctx,
                                                       float* __restrict__ lse, int items, int QG) {
  constexpr int LD = DP + 1, KS = DP / 4, DT = DP / 16;
  __shared__ float ksh[QC * LD], vsh[QC * LD];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, col = lane & 15, kq = lane >> 4;
  const size_t ldq = (size_t)3 * NH * DP;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int qg = item % QG, h = (item / QG) % NH, b = item / (QG * NH);
    const int len = min(max(lens[b], 0), L);
    const int q = (qg * 4 + w) * 16 + col;                       // the lane's query
    const bool qlive = q < len, wlive = (qg * 4 + w) * 16 < len;
    float qf[KS];
    load_frag<DP>(qkv + ((size_t)(qlive ? q : 0) * B + b) * ldq + h * DP, qlive, kq, qf);
    f32x4 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;
    const int chunks = qg * QC < len ? (len + QC - 1) / QC : 0;
    for (int c = 0; c < chunks; ++c) {
      stage<DP>(ksh, qkv + (NH + h) * DP, ldq, c * QC, len, B, b);
      stage<DP>(vsh, qkv + (2 * NH + h) * DP, ldq, c * QC, len, B, b);
      __syncthreads();
      if (wlive) {
        for (int kt = 0; kt < 4 && c * QC + kt * 16 < len; ++kt) {
          const int jv = len - (c * QC + kt * 16);               // live keys of the tile, >= 1
          const float* kk = ksh + kt * 16 * LD;
          const float* vv = vsh + kt * 16 * LD;
          f32x4 sc = f32x4{0.f, 0.f, 0.f, 0.f};                  // S^T[key 4 kq + i][query col]
#pragma unroll
          for (int s = 0; s < KS; ++s)
            sc = __builtin_amdgcn_mfma_f32_16x16x4f32(kk[col * LD + frag_d(s, kq)], qf[s], sc, 0, 0, 0);
          float mx = -INFINITY;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            // the product rounded on its own (no fma with the subtraction), here and in the backward, so that the
            // backward's s - lse is the forward's
            sc[i] = 4 * kq + i < jv ? mul_rn(sc[i], scale) : -INFINITY;
            mx = fmaxf(mx, sc[i]);
          }
          const float mn = fmaxf(m, xor_max(mx)), alpha = exp2f((m - mn) * LOG2E);
          float ps = 0.f;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            sc[i] = exp2f((sc[i] - mn) * LOG2E);
            ps += sc[i];
          }
          l = l * alpha + xor_sum(ps);
          m = mn;
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) o[dt] *= alpha;
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
              o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(vv[(4 * kq + r) * LD + dt * 16 + col], sc[r], o[dt], 0, 0, 0);
        }
      }
      __syncthreads();
    }
    if (q < L) {   // the lane holds O^T[d = 16 dt + 4 kq + i][query col]
      const size_t row = ((size_t)q * B + b) * NH + h;
      const float inv = 1.f / l;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) store4(ctx + row * DP + 16 * dt + 4 * kq, o[dt], inv, qlive);
      if (kq == 0) lse[row] = qlive ? m + log2f(l) * LN2 : 0.f;
    }
  }
}

template <int DP>
__global__ __launch_bounds__(256) void attn_bwd_kernel(const float* __restrict__ qkv, const int* __restrict__ lens,
                                                       const float* __restrict__ ctx, const float* __restrict__ lse,
                                                       const float* __restrict__ dctx, int L, int B, int NH,
                                                       float scale, float* __restrict__ dqkv, int items, int QG) {
  constexpr int LD = DP + 1, KS = DP / 4, DT = DP / 16;
  __shared__ float sha[QC * LD], shb[QC * LD];       // role 0: K, V; role 1: Q, dO
  __shared__ float lsesh[QC];                        // role 1: lse of the chunk's queries
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, col = lane & 15, kq = lane >> 4;
  const size_t ldq = (size_t)3 * NH * DP;
  const bool dq_role = blockIdx.y == 0;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int g = item % QG, h = (item / QG) % NH, b = item / (QG * NH);
    const int len = min(max(lens[b], 0), L);
    const int t = (g * 4 + w) * 16 + col;                        // the lane's own row: a query (role 0) or a key
    const bool tlive = t < len, wlive = (g * 4 + w) * 16 < len;
    const size_t trow = (size_t)(tlive ? t : 0) * B + b;
    const int chunks = g * QC < len ? (len + QC - 1) / QC : 0;
    f32x4 acc0[DT], acc1[DT];                                    // role 0: dQ^T, -; role 1: dK^T, dV^T
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc0[dt] = acc1[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float fa[KS], fb[KS];                                        // role 0: Q, dO; role 1: K, V
    if (dq_role) {
      float cf[KS];
      load_frag<DP>(qkv + trow * ldq + h * DP, tlive, kq, fa);
      load_frag<DP>(dctx + (trow * NH + h) * DP, tlive, kq, fb);
      load_frag<DP>(ctx + (trow * NH + h) * DP, tlive, kq, cf);
      f32x4 dl = f32x4{0.f, 0.f, 0.f, 0.f};                      // [query 4 kq + i][query col] of ctx dO^T
#pragma unroll
      for (int s = 0; s < KS; ++s) dl = __builtin_amdgcn_mfma_f32_16x16x4f32(cf[s], fb[s], dl, 0, 0, 0);
      const int ci = col & 3;
      const float diag = ci == 0 ? dl[0] : ci == 1 ? dl[1] : ci == 2 ? dl[2] : dl[3];
      const float delta = __shfl(diag, (col >> 2) * 16 + col, 64);   // the lane that holds row col of column col
      const float lq = tlive ? lse[trow * NH + h] : 0.f;
      for (int c = 0; c < chunks; ++c) {
        stage<DP>(sha, qkv + (NH + h) * DP, ldq, c * QC, len, B, b);
        stage<DP>(shb, qkv + (2 * NH + h) * DP, ldq, c * QC, len, B, b);
        __syncthreads();
        if (wlive) {
          for (int kt = 0; kt < 4 && c * QC + kt * 16 < len; ++kt) {
            const int jv = len - (c * QC + kt * 16);
            const float* kk = sha + kt * 16 * LD;
            const float* vv = shb + kt * 16 * LD;
            f32x4 sc = f32x4{0.f, 0.f, 0.f, 0.f}, dp = sc;       // S^T, dP^T [key 4 kq + i][query col]
#pragma unroll
            for (int s = 0; s < KS; ++s) {
              const int d = col * LD + frag_d(s, kq);
              sc = __builtin_amdgcn_mfma_f32_16x16x4f32(kk[d], fa[s], sc, 0, 0, 0);
              dp = __builtin_amdgcn_mfma_f32_16x16x4f32(vv[d], fb[s], dp, 0, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float p = 4 * kq + i < jv ? exp2f((mul_rn(sc[i], scale) - lq) * LOG2E) : 0.f;
              sc[i] = p * (dp[i] - delta);                       // dS^T
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
              for (int dt = 0; dt < DT; ++dt)
                acc0[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(kk[(4 * kq + r) * LD + dt * 16 + col], sc[r], acc0[dt],
                                                                0, 0, 0);
          }
        }
        __syncthreads();
      }
    } else {
      load_frag<DP>(qkv + trow * ldq + (NH + h) * DP, tlive, kq, fa);
      load_frag<DP>(qkv + trow * ldq + (2 * NH + h) * DP, tlive, kq, fb);
      for (int c = 0; c < chunks; ++c) {
        stage<DP>(sha, qkv + h * DP, ldq, c * QC, len, B, b);
        stage<DP>(shb, dctx + h * DP, (size_t)NH * DP, c * QC, len, B, b);
        if (threadIdx.x < QC) {
          const int q = c * QC + threadIdx.x;
          lsesh[threadIdx.x] = q < len ? lse[((size_t)q * B + b) * NH + h] : 0.f;
        }
        __syncthreads();
        if (wlive) {
          for (int qt = 0; qt < 4 && c * QC + qt * 16 < len; ++qt) {
            const int q0 = c * QC + qt * 16, qv = len - q0;
            const float* qq = sha + qt * 16 * LD;
            const float* dd = shb + qt * 16 * LD;
            float cf[KS];                                        // ctx of query q0 + col
            const bool ql = q0 + col < len;
            load_frag<DP>(ctx + (((size_t)(ql ? q0 + col : 0) * B + b) * NH + h) * DP, ql, kq, cf);
            f32x4 sc = f32x4{0.f, 0.f, 0.f, 0.f}, dp = sc, dl = sc;   // S, dP [query 4 kq + i][key col]; dO ctx^T
#pragma unroll
            for (int s = 0; s < KS; ++s) {
              const int d = col * LD + frag_d(s, kq);
              sc = __builtin_amdgcn_mfma_f32_16x16x4f32(qq[d], fa[s], sc, 0, 0, 0);
              dp = __builtin_amdgcn_mfma_f32_16x16x4f32(dd[d], fb[s], dp, 0, 0, 0);
              dl = __builtin_amdgcn_mfma_f32_16x16x4f32(dd[d], cf[s], dl, 0, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int qi = 4 * kq + i;                         // delta of query qi: row qi of column qi
              const float delta = __shfl(dl[i], kq * 16 + qi, 64);
              const float p = qi < qv && tlive ? exp2f((mul_rn(sc[i], scale) - lsesh[qt * 16 + qi]) * LOG2E) : 0.f;
              sc[i] = p;
              dp[i] = p * (dp[i] - delta);                       // dS
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
              for (int dt = 0; dt < DT; ++dt) {
                const int d = (4 * kq + r) * LD + dt * 16 + col;
                acc0[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(qq[d], dp[r], acc0[dt], 0, 0, 0);
                acc1[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(dd[d], sc[r], acc1[dt], 0, 0, 0);
              }
          }
        }
        __syncthreads();
      }
    }
    if (t < L) {   // the lane holds d = 16 dt + 4 kq + i of its own row
      float* dst = dqkv + ((size_t)t * B + b) * ldq + h * DP + 4 * kq;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        if (dq_role) {
          store4(dst + 16 * dt, acc0[dt], scale, tlive);
        } else {
          store4(dst + NH * DP + 16 * dt, acc0[dt], scale, tlive);
          store4(dst + 2 * NH * DP + 16 * dt, acc1[dt], 1.f, tlive);
        }
      }
    }
  }
}

bool attn_extents_ok(int L, int B, int NH, int DP) {
  return L >= 1 && B >= 1 && NH >= 1 && NH <= 8 && (DP == 16 || DP == 32) &&
         (long long)B * NH * rk_cdiv(L, QC) < (1ll << 30);
}

}  // namespace

// ctx [n][NH][DP] and lse [n][NH] of qkv [n][3][NH][DP], n = L * B time-major rows, keys masked from lens[b] on
extern "C" int rk_attn_fwd(const float* qkv, const int* lens, int L, int B, int NH, int DP, float scale, float* ctx,
                           float* lse, void* stream) {
  if (L <= 0 || B <= 0) return RK_OK;
  if (!attn_extents_ok(L, B, NH, DP)) return RK_EBADARG;
  const int QG = rk_cdiv(L, QC), items = B * NH * QG, G = items < GRID_CAP ? items : GRID_CAP;
  if (DP == 16)
    hipLaunchKernelGGL(attn_fwd_kernel<16>, dim3(G), dim3(256), 0, (hipStream_t)stream, qkv, lens, L, B, NH, scale,
                       ctx, lse, items, QG);
  else
    hipLaunchKernelGGL(attn_fwd_kernel<32>, dim3(G), dim3(256), 0, (hipStream_t)stream, qkv, lens, L, B, NH, scale,
                       ctx, lse, items, QG);
  RK_LAUNCH_CHECK();
  return RK_OK;
}

// dqkv [n][3][NH][DP] (fully written) from the forward's ctx and lse and the upstream dctx
extern "C" int rk_attn_bwd(const float* qkv, const int* lens, const float* ctx, const float* lse, const float* dctx,
                           int L, int B, int NH, int DP, float scale, float* dqkv, void* stream) {
  if (L <= 0 || B <= 0) return RK_OK;
  if (!attn_extents_ok(L, B, NH, DP)) return RK_EBADARG;
  const int QG = rk_cdiv(L, QC), items = B * NH * QG, G = items < GRID_CAP ? items : GRID_CAP;
  if (DP == 16)
    hipLaunchKernelGGL(attn_bwd_kernel<16>, dim3(G, 2), dim3(256), 0, (hipStream_t)stream, qkv, lens, ctx, lse, dctx,
                       L, B, NH, scale, dqkv, items, QG);
  else
    hipLaunchKernelGGL(attn_bwd_kernel<32>, dim3(G, 2), dim3(256), 0, (hipStream_t)stream, qkv, lens, ctx, lse, dctx,
                       L, B, NH, scale, dqkv, items, QG);
  RK_LAUNCH_CHECK();
  return RK_OK;
}
