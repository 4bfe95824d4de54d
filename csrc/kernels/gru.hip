// Persistent bidirectional GRU recurrence for gfx950, fp32 (PyBiGru / PyBiGruCrf through engine/tagger.py;
// nn.GRU(bidirectional=True) on a padded batch, gate blocks [r | z | n] of HP each, HP = 64 or 128):
//
//   r = sigm(a_r + W_hr h + b_hr)      z = sigm(a_z + W_hz h + b_hz)
//   q = W_hn h + b_hn                  n = tanh(a_n + r * q)            h' = (1 - z) * n + z * h
//
// a = x W_ih^T + b_ih has no time dependence and is one plain GEMM outside.  Unlike the LSTM (lstm.hip) the
// recurrent product cannot be folded into it: q is multiplied by r before a_n is added, so the kernel takes
// b_hh itself and keeps q in an accumulator of its own.  The launch shape is the LSTM's: ONE launch runs the
// whole sequence; a workgroup owns (direction d, 16 batch rows); wave w owns units [w*HP/4, (w+1)*HP/4) of all
// three gates, so one lane's v_mfma_f32_16x16x4_f32 outputs hold r, z and q of the same (row, unit) and the
// update is lane-local.  h_{t-1} of the lane's own (row, unit) stays in a register (fp32, the z * h term, where
// the LSTM keeps c); the MFMA operand copy of h_{t-1} goes through a double-buffered LDS tile, one barrier per
// step.  The next step's a rows are prefetched before this step's MFMAs.  Rows b >= B are held at zero; padded
// units stay exactly 0 (zero weights and biases: r = z = 1/2, q = 0, n = 0, h' = 1/2 * 0 + 1/2 * 0).
//
// Where W_hh lives.  A lane's share of W_hh is 3 gates x UB unit blocks x HP/4 k = 48 floats at HP = 64 and 192
// at HP = 128 (the LSTM's four gates: 64 and 256).  A 256-thread workgroup puts one wave on each SIMD, so with one
// workgroup per CU a wave may use the whole unified file of 512 registers: 192 + accumulators + prefetch fit,
// the LSTM's 256 do not (that is why lstm_fwd32_kernel<128> re-reads W_hh from L2 every step).  Both GRU kernels
// therefore load their fragments once and keep them in registers for the whole sequence, at both HP: the
// forward W_hh [3HP][HP] rows, the backward W_hh^T [HP][3HP] rows (also 48 / 192 floats per lane).  The
// compiler's resource report (-Rpass-analysis=kernel-resource-usage) shows no scratch for any of the four
// instantiations: forward 110 VGPRs + 20 AGPRs at HP 64 and 256 + 74 at HP 128, backward 92 + 8 and 248 + 16,
// one wave per SIMD at HP 128.  Measured on an MI355X at (T 40, B 32, HP 128) against the same kernels re-reading
// their fragments from L2 every step: forward 208 us against 363 us, backward 222 us against 328 us
// (profiles/gru_whh_residency_ab.json); the re-read form was deleted.
//
// Backward (BPTT), reverse time, dh = dhout_t + dh_rec, h_prev read from hout (zero at the first step):
//   da_n = dh (1 - z)(1 - n^2)      da_z = dh (h_prev - n) z (1 - z)      da_r = da_n q r (1 - r)
//   dgin = [da_r | da_z | da_n]     dgh = [da_r | da_z | da_n r]          dh_rec' = dh z + dgh . W_hh
// The dh z carry is lane-local (where the LSTM carries dc); dgh is the MFMA operand, through a double-buffered
// LDS tile [16][3HP + 4]; two accumulator sets per unit block hide the dependent-MFMA latency.  dgin and dgh both
// go to global memory: dW_ih = dgin^T x, dW_hh = dgh^T h_prev, db_ih = colsum(dgin), db_hh = colsum(dgh) are
// plain GEMMs and column sums outside.
//
// Layouts:
//   gin   fp32 [T][B][2][3HP]  input projection incl. b_ih only      whh  fp32 [2][3HP][HP]    bhh fp32 [2][3HP]
//   hout  fp32 [T][B][2][HP]                                         whhT fp32 [2][HP][3HP]
//   gsave fp32 [T][B][2][3HP]  activated r, z, n                     qsave fp32 [T][B][2][HP]  (W_hn h + b_hn)
//   dhout fp32 [T][B][2][HP]   dgin fp32 [T][B][2][3HP]   dgh fp32 [T][B][2][3HP]
#include "common.h"

namespace {

constexpr int GROWS = 16;

RK_DEV float sigm(float x) { return 1.0f / (1.0f + __expf(-x)); }
RK_DEV float tanh_f(float x) {
  const float e = __expf(-2.0f * fabsf(x));
  const float t = (1.0f - e) / (1.0f + e);
  return x < 0.f ? -t : t;
}

// lane group kq = lane >> 4 supplies k in [kq*KQ, (kq+1)*KQ) (a permuted K order, so both operands stream as
// float4); D[row kq*4 + i][unit col] is the lane's, as in lstm.hip.
template <int HP>
__global__ __launch_bounds__(256) void gru_fwd32_kernel(const float* __restrict__ gin, const float* __restrict__ whh,
                                                        const float* __restrict__ bhh, int T, int B,
                                                        float* __restrict__ hout, float* __restrict__ gsave,
                                                        float* __restrict__ qsave) {
  constexpr int UB = HP / 64;      // 16-unit blocks per wave
  constexpr int KQ = HP / 4;       // k per lane group
  constexpr int G3 = 3 * HP;
  constexpr int LD = HP + 4;
  __shared__ __attribute__((aligned(16))) float hs[2][GROWS][LD];
  const int d = blockIdx.y, r0 = blockIdx.x * GROWS;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = lane & 15, kq = lane >> 4;
  const float* wd = whh + (long long)d * G3 * HP;
  f32x4 wres[3][UB][KQ / 4];       // W_hh[g*HP + unit][kq*KQ ..], resident for the whole sequence
  float bh[3][UB];
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int ub = 0; ub < UB; ++ub) {
      const int unit = w * (HP / 4) + ub * 16 + col;
      bh[g][ub] = bhh[d * G3 + g * HP + unit];
#pragma unroll
      for (int k4 = 0; k4 < KQ / 4; ++k4)
        wres[g][ub][k4] = *(const f32x4*)(wd + (long long)(g * HP + unit) * HP + kq * KQ + 4 * k4);
    }
  for (int i = threadIdx.x; i < GROWS * LD; i += 256) (&hs[0][0][0])[i] = 0.f;
  float h[UB][4];
#pragma unroll
  for (int ub = 0; ub < UB; ++ub)
#pragma unroll
    for (int i = 0; i < 4; ++i) h[ub][i] = 0.f;
  auto gin_at = [&](int t, int row, int g, int unit) -> float {
    const int b = r0 + row;
    return b < B ? gin[(((long long)t * B + b) * 2 + d) * G3 + g * HP + unit] : 0.f;
  };
  float pre[3][UB][4];
  const int t_first = d == 0 ? 0 : T - 1;
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int ub = 0; ub < UB; ++ub)
#pragma unroll
      for (int i = 0; i < 4; ++i) pre[g][ub][i] = gin_at(t_first, kq * 4 + i, g, w * (HP / 4) + ub * 16 + col);
  __syncthreads();
  int cur = 0;
  for (int s = 0; s < T; ++s) {
    const int t = d == 0 ? s : T - 1 - s;
    // r, z start from a + b_hh; q from b_hn alone (a_n joins after the product with r)
    f32x4 acc[3][UB];
    float an[UB][4];
#pragma unroll
    for (int ub = 0; ub < UB; ++ub) {
#pragma unroll
      for (int g = 0; g < 2; ++g)
        acc[g][ub] = f32x4{pre[g][ub][0] + bh[g][ub], pre[g][ub][1] + bh[g][ub], pre[g][ub][2] + bh[g][ub],
                           pre[g][ub][3] + bh[g][ub]};
      acc[2][ub] = f32x4{bh[2][ub], bh[2][ub], bh[2][ub], bh[2][ub]};
#pragma unroll
      for (int i = 0; i < 4; ++i) an[ub][i] = pre[2][ub][i];
    }
    if (s + 1 < T) {   // prefetch the next step's projection while the MFMAs run
      const int tn = d == 0 ? t + 1 : t - 1;
#pragma unroll
      for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int ub = 0; ub < UB; ++ub)
#pragma unroll
          for (int i = 0; i < 4; ++i) pre[g][ub][i] = gin_at(tn, kq * 4 + i, g, w * (HP / 4) + ub * 16 + col);
    }
#pragma unroll
    for (int k4 = 0; k4 < KQ / 4; ++k4) {   // fully unrolled: the resident weights stay in registers
      const f32x4 a = *(const f32x4*)&hs[cur][col][kq * KQ + 4 * k4];
#pragma unroll
      for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int ub = 0; ub < UB; ++ub)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            acc[g][ub] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], wres[g][ub][k4][e], acc[g][ub], 0, 0, 0);
    }
#pragma unroll
    for (int ub = 0; ub < UB; ++ub) {
      const int unit = w * (HP / 4) + ub * 16 + col;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = kq * 4 + i, b = r0 + row;
        const float rg = sigm(acc[0][ub][i]), zg = sigm(acc[1][ub][i]), q = acc[2][ub][i];
        const float ng = tanh_f(an[ub][i] + rg * q);
        const float hn = b < B ? (1.f - zg) * ng + zg * h[ub][i] : 0.f;
        h[ub][i] = hn;
        hs[cur ^ 1][row][unit] = hn;
        if (b < B) {
          const long long o = ((long long)t * B + b) * 2 + d;
          hout[o * HP + unit] = hn;
          qsave[o * HP + unit] = q;
          float* gp = gsave + o * G3 + unit;
          gp[0] = rg; gp[HP] = zg; gp[2 * HP] = ng;
        }
      }
    }
    __syncthreads();
    cur ^= 1;
  }
}

template <int HP>
__global__ __launch_bounds__(256) void gru_bwd32_kernel(const float* __restrict__ whhT, int T, int B,
                                                        const float* __restrict__ dhout,
                                                        const float* __restrict__ hout,
                                                        const float* __restrict__ gsave,
                                                        const float* __restrict__ qsave, float* __restrict__ dgin,
                                                        float* __restrict__ dgh) {
  constexpr int UB = HP / 64;
  constexpr int G3 = 3 * HP;
  constexpr int KQ = G3 / 4;       // k per lane group of dh_rec = dgh [16 x 3HP] . W_hh [3HP x HP]
  constexpr int LD = G3 + 4;
  __shared__ __attribute__((aligned(16))) float gs[2][GROWS][LD];
  const int d = blockIdx.y, r0 = blockIdx.x * GROWS;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = lane & 15, kq = lane >> 4;
  const float* wt = whhT + (long long)d * HP * G3;
  f32x4 wres[UB][KQ / 4];          // W_hh^T[unit][kq*KQ ..], resident for the whole sequence
#pragma unroll
  for (int ub = 0; ub < UB; ++ub)
#pragma unroll
    for (int k4 = 0; k4 < KQ / 4; ++k4)
      wres[ub][k4] = *(const f32x4*)(wt + (long long)(w * (HP / 4) + ub * 16 + col) * G3 + kq * KQ + 4 * k4);
  float dhz[UB][4];                // dh * z of the step before: the lane-local part of dh_rec
  f32x4 dhr[UB];
#pragma unroll
  for (int ub = 0; ub < UB; ++ub) {
    dhr[ub] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) dhz[ub][i] = 0.f;
  }
  int cur = 0;
  for (int s = 0; s < T; ++s) {
    const int t = d == 0 ? T - 1 - s : s;            // reverse of the forward order
    const int tp = d == 0 ? t - 1 : t + 1;           // the forward's previous step
    const bool has_prev = d == 0 ? t > 0 : t < T - 1;
#pragma unroll
    for (int ub = 0; ub < UB; ++ub) {
      const int unit = w * (HP / 4) + ub * 16 + col;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = kq * 4 + i, b = r0 + row;
        float dar = 0.f, daz = 0.f, dan = 0.f, dqn = 0.f;
        if (b < B) {
          const long long o = ((long long)t * B + b) * 2 + d;
          const float* gp = gsave + o * G3 + unit;
          const float rg = gp[0], zg = gp[HP], ng = gp[2 * HP];
          const float q = qsave[o * HP + unit];
          const float hp = has_prev ? hout[(((long long)tp * B + b) * 2 + d) * HP + unit] : 0.f;
          const float dh = dhout[o * HP + unit] + dhr[ub][i] + dhz[ub][i];
          dan = dh * (1.f - zg) * (1.f - ng * ng);
          daz = dh * (hp - ng) * zg * (1.f - zg);
          dar = dan * q * rg * (1.f - rg);
          dqn = dan * rg;
          dhz[ub][i] = dh * zg;
          float* dp = dgin + o * G3 + unit;
          dp[0] = dar; dp[HP] = daz; dp[2 * HP] = dan;
          float* hp2 = dgh + o * G3 + unit;
          hp2[0] = dar; hp2[HP] = daz; hp2[2 * HP] = dqn;
        }
        gs[cur][row][unit] = dar;
        gs[cur][row][HP + unit] = daz;
        gs[cur][row][2 * HP + unit] = dqn;
      }
    }
    __syncthreads();
    // dh_rec[row][unit] = sum_k dgh[row][k] * W_hh[k][unit]
    f32x4 acc[2][UB];
#pragma unroll
    for (int ub = 0; ub < UB; ++ub) acc[0][ub] = acc[1][ub] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k4 = 0; k4 < KQ / 4; ++k4) {
      const f32x4 a = *(const f32x4*)&gs[cur][col][kq * KQ + 4 * k4];
#pragma unroll
      for (int ub = 0; ub < UB; ++ub)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          acc[e & 1][ub] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], wres[ub][k4][e], acc[e & 1][ub], 0, 0, 0);
    }
#pragma unroll
    for (int ub = 0; ub < UB; ++ub) dhr[ub] = acc[0][ub] + acc[1][ub];
    cur ^= 1;   // the other buffer is free: everyone passed this step's barrier after reading it
  }
}

}  // namespace

// whh fp32 [2][3HP][HP], bhh fp32 [2][3HP]; gin carries b_ih only
extern "C" int rk_gru_fwd32(const float* gin, const float* whh, const float* bhh, int T, int B, int HP, float* hout,
                            float* gsave, float* qsave, void* stream) {
  if (T <= 0 || B <= 0) return RK_OK;
  const dim3 grid(rk_cdiv(B, GROWS), 2), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (HP == 64)
    hipLaunchKernelGGL(gru_fwd32_kernel<64>, grid, block, 0, s, gin, whh, bhh, T, B, hout, gsave, qsave);
  else if (HP == 128)
    hipLaunchKernelGGL(gru_fwd32_kernel<128>, grid, block, 0, s, gin, whh, bhh, T, B, hout, gsave, qsave);
  else
    return RK_EUNSUPPORTED;
  RK_LAUNCH_CHECK();
  return RK_OK;
}

// whhT fp32 [2][HP][3HP]; hout, gsave, qsave as the forward wrote them
extern "C" int rk_gru_bwd32(const float* whhT, int T, int B, int HP, const float* dhout, const float* hout,
                            const float* gsave, const float* qsave, float* dgin, float* dgh, void* stream) {
  if (T <= 0 || B <= 0) return RK_OK;
  const dim3 grid(rk_cdiv(B, GROWS), 2), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (HP == 64)
    hipLaunchKernelGGL(gru_bwd32_kernel<64>, grid, block, 0, s, whhT, T, B, dhout, hout, gsave, qsave, dgin, dgh);
  else if (HP == 128)
    hipLaunchKernelGGL(gru_bwd32_kernel<128>, grid, block, 0, s, whhT, T, B, dhout, hout, gsave, qsave, dgin, dgh);
  else
    return RK_EUNSUPPORTED;
  RK_LAUNCH_CHECK();
  return RK_OK;
}
