// Inverted dropout for the conv-net training step (engine/convnet.py), in place, with nothing stored: the
// multipliers are a pure function of (seed, call site, step, epoch, element), so the backward pass runs the same
// launcher on the gradient that arrives at the dropped tensor and regenerates them.
//
//   * element i belongs to quad q = i / 4 and uses word i % 4 of
//     philox4x32_10(counter (q, site, *step, *epoch), key (seed low word, seed high word));
//   * it is kept iff u01(word) >= p; out = keep ? x * inv_keep : 0 with inv_keep = 1 / (1 - p) formed in fp32 by
//     the launcher.  fp32: one fp32 multiply.  bf16: the product in fp32, rounded to nearest-even;
//   * a dropped element is written as zero by selection, never as x * 0: a dropped inf / NaN becomes 0;
//   * step / epoch are device words read by the kernel (null: 0), so a replayed hipGraph draws the multipliers of
//     whatever they hold at replay time.
//
// One thread per 16-B vector and no more Philox blocks than it needs: an fp32 vector is one quad (one block), a
// bf16 vector two quads (two blocks).  ops/dropout.py is the host twin of the draws.
#include "common.h"
#include "philox.h"

namespace {

RK_DEV uint32_t word_or_zero(const int* __restrict__ p) { return p ? (uint32_t)p[0] : 0u; }

__global__ __launch_bounds__(256) void dropout_f32_kernel(float* __restrict__ x, long long nvec, float p,
                                                          float inv_keep, uint32_t k0, uint32_t k1, uint32_t site,
                                                          const int* __restrict__ step,
                                                          const int* __restrict__ epoch) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nvec) return;
  const U4 r = philox4x32_10((uint32_t)i, site, word_or_zero(step), word_or_zero(epoch), k0, k1);
  f32x4 v = ((const f32x4*)x)[i];
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = u01(r.v[e]) >= p ? v[e] * inv_keep : 0.f;
  ((f32x4*)x)[i] = v;
}

__global__ __launch_bounds__(256) void dropout_bf16_kernel(bf16* __restrict__ x, long long nvec, float p,
                                                           float inv_keep, uint32_t k0, uint32_t k1, uint32_t site,
                                                           const int* __restrict__ step,
                                                           const int* __restrict__ epoch) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nvec) return;
  const uint32_t st = word_or_zero(step), ep = word_or_zero(epoch);
  const U4 r0 = philox4x32_10((uint32_t)(2 * i), site, st, ep, k0, k1);
  const U4 r1 = philox4x32_10((uint32_t)(2 * i + 1), site, st, ep, k0, k1);
  bf16x8 v = __builtin_bit_cast(bf16x8, ((const uint4*)x)[i]);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    v[e] = u01(r0.v[e]) >= p ? f2bf(bf2f(v[e]) * inv_keep) : f2bf(0.f);
    v[4 + e] = u01(r1.v[e]) >= p ? f2bf(bf2f(v[4 + e]) * inv_keep) : f2bf(0.f);
  }
  ((uint4*)x)[i] = __builtin_bit_cast(uint4, v);
}

}  // namespace

// x [n] (fp32, or bf16 when is_bf16) *= the multipliers of (seed, site, *step, *epoch), in place; x 16-B aligned,
// n a multiple of the elements per 16-B vector, n / 4 < 2^32 (the quad index is one counter word)
extern "C" int rk_dropout(void* x, long long n, int is_bf16, float p, unsigned long long seed, unsigned site,
                          const int* step, const int* epoch, void* stream) {
  const int vw = is_bf16 ? 8 : 4;
  if (!(p >= 0.f && p < 1.f)) return RK_EBADARG;   // NaN fails both comparisons
  if (n < 0 || n % vw || n / 4 >= (1LL << 32)) return RK_EBADARG;
  if (n == 0) return RK_OK;
  if (!x || ((uintptr_t)x & 15)) return RK_EBADARG;
  const long long nvec = n / vw;
  const float inv_keep = 1.0f / (1.0f - p);
  const dim3 grid((unsigned)((nvec + 255) / 256)), block(256);
  if (is_bf16)
    hipLaunchKernelGGL(dropout_bf16_kernel, grid, block, 0, (hipStream_t)stream, (bf16*)x, nvec, p, inv_keep,
                       (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)site, step, epoch);
  else
    hipLaunchKernelGGL(dropout_f32_kernel, grid, block, 0, (hipStream_t)stream, (float*)x, nvec, p, inv_keep,
                       (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)site, step, epoch);
  RK_LAUNCH_CHECK();
  return RK_OK;
}
