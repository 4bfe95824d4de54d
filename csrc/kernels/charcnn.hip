// Fused character-CNN word features for gfx950, fp32 (PyBiLstmChar / PyBiLstmCharCrf through engine/tagger.py; the
// "CNN" of BiLSTM-CNN-CRF, Ma & Hovy 2016): embedding gather -> width-3 convolution -> max over the word's
// positions -> bias -> dropout, as one launch forward and two backward, without ever writing the convolution's
// input or output to memory.
//
//   a token carries C = 16 character ids (uint8, 0 = padding, the word is a prefix), len = #non-zero ids
//   X[p] = cemb[id[p]] for p < len and id[p] < CV, else 0; X[-1] = X[16] = 0
//   conv[p][f] = sum_{k<3} sum_e X[p+k-1][e] Wc[f][k][e]        feat[f] = bc[f] + max_{p<len} conv[p][f]
//   amax[f] = the first p attaining the maximum (-1 and feat = 0 for len = 0)
//
// Forward (charcnn_fwd_kernel<EcP, NCT>, FP = 16 NCT filters).  A wave per word, waves stride over the words of a
// capped grid.  The 16 positions are the 16 rows of a v_mfma_f32_16x16x4_f32 tile: the word's [18][EcP] window
// (rows 0 and 17 the zero padding) sits in LDS and the A operand of tap k is that window read at row offset k, so
// there is no im2col.  The character table is staged once per workgroup in LDS (CV EcP 4 <= 32 KB): the gather never
// leaves the CU.  The B fragments of Wc (NCT x 3 x EcP/4 <= 96 floats a lane) stay in registers for all of the
// wave's words.  Rows p >= len are masked to -inf; a lane holds 4 rows of a column, so the max over positions is 4
// in-lane values and two cross-lane steps (xor 16, 32), each keeping the lower index on a tie.  Lane group g then
// finishes column tile g: bias, the Philox dropout multiplier keyed as rk_tag_embed_fwd keys it (counter = element
// / 4, stream id, device step), xc, mask and amax (int32).  The window row stride is EcP + 1 floats: the A reads of
// 16 rows at one k fall on 16 different banks.
//
// Backward (charcnn_bwd_kernel<EcP, NCT>, then charcnn_fold_kernel), bit-reproducible, no float atomics anywhere.
//   g[f] = dxc[f] mask[f].  dWc, dbc: a lane per filter keeps dWc[f][3][EcP] and dbc[f] in registers over all of
//   its wave's words and adds g[f] X[amax_f + k - 1][.] from the window: lane-local.  dX [16][EcP] of a word is an
//   MFMA with a one-hot-row A operand (A_k[q][f] = g[f] where amax_f + k - 1 == q) against the resident Wc taps, all
//   three taps into one D tile; rows outside 0..15 never match a q and drop out.  dcemb: the workgroup owns an LDS
//   table [CV][EcP]; its waves stage their dX rows and row ids, and after a barrier thread (e, id % (256/EcP)) walks
//   the 4 x 16 staged rows in fixed order (wave 0..3, row 0..15) adding those of its ids: one owner per address, a
//   fixed order, so "aa" never has two lanes on one address.  The table is the reason the backward gathers X from
//   global memory (L2-resident) rather than staging cemb as well: two 32 KB tables and the windows pass 64 KB.
//   At the end every workgroup writes its table into ws, folds its four waves' dWc | dbc through the table's LDS
//   (wave 0 to 3 in turn, filter-minor so LDS and global accesses are contiguous) and writes that too; the fold
//   kernel sums the G partials in a fixed order (fp64 accumulators) into dwc, dbc and dcemb, writing every element.
//   rk_reduce_slabs was not used for it: the dWc partial is transposed, the outputs are three tensors, and its
//   one-thread-per-element walk over the partials is latency-bound here (a first version of this fold that summed
//   512 wave partials a thread took 149 us in the step; see profiles/charcnn_tagger_step.json).
//
// Deviations from the suggested design: the waves' dWc | dbc are folded inside the workgroup, so ws holds G partials
// and not 4 G; the in-workgroup table add is one barrier pair per word round with the addresses dealt over all 256
// threads, not four wave turns (same fixed order per address, a quarter of the barriers).  amax is int32.
//
// Resource report (-Rpass-analysis=kernel-resource-usage, gfx950): ScratchSize 0 for all 17 kernels.
//   forward  <16, 1..4>: 41 / 57 / 71 / 83 VGPRs + 4 / 8 / 12 / 20 AGPRs, LDS 21280 B
//   forward  <32, 1..4>: 53 / 81 / 107 / 131 VGPRs + 4 / 8 / 12 / 20 AGPRs, LDS 42272 B, 3 waves / SIMD
//   backward <16, 1..4>: 94 / 112 / 124 / 136 VGPRs + 4 AGPRs, LDS 27936 B
//   backward <32, 1..4>: 160 / 184 / 208 / 232 VGPRs + 8 AGPRs, LDS 53024 B, 2 waves / SIMD (one workgroup a CU)
//   fold: 43 VGPRs, LDS 2048 B
//
// Layouts: chars uint8 [n][16]   cemb fp32 [CV][EcP]   wc fp32 [FP][3][EcP]   bc fp32 [FP]
//          xc, mask, dxc fp32 [n][FP]   amax int32 [n][FP]   EcP in {16, 32}, FP in {16, 32, 48, 64}, CV <= 256
//          ws: [G][3 EcP FP + FP] dWc | dbc partials, then [G][CV EcP] tables, G = min(ceil(n / 4), 128) workgroups
#include "common.h"
#include "philox.h"

namespace {

constexpr int CC = 16;        // characters per token
constexpr int CVMAX = 256;    // rows of the character table
constexpr int GRID_CAP = 128;

// LDS traffic between the lanes of one wave: DS instructions of a wave execute in order; this keeps the compiler
// from moving them across
RK_DEV void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// lane l gets id[l & 15] of the token; len = the number of non-zero ids
RK_DEV int load_ids(const uint8_t* __restrict__ chars, int tok, int lane, int& len) {
  const int id = chars[(long long)tok * CC + (lane & 15)];
  len = __popcll(__ballot(lane < 16 && id != 0));
  return id;
}

// window rows 1..16 = X[0..15]: lane l fills a quarter of row p = l >> 2 from table [CV][EcP]
template <int EcP>
RK_DEV void fill_window(float* win, const float* table, int id, int len, int CV, int lane) {
  constexpr int LD = EcP + 1, Q = EcP / 4;
  const int p = lane >> 2, c0 = (lane & 3) * Q;
  const int pid = __shfl(id, p, 64);
  const bool live = p < len && pid < CV;
  const float* src = table + (live ? pid : 0) * EcP + c0;
#pragma unroll
  for (int j = 0; j < Q; ++j) win[(p + 1) * LD + c0 + j] = live ? src[j] : 0.f;
}

template <int EcP, int NCT>
__global__ __launch_bounds__(256) void charcnn_fwd_kernel(const uint8_t* __restrict__ chars,
                                                          const float* __restrict__ cemb, const float* __restrict__ wc,
                                                          const float* __restrict__ bc, int n, int CV, float p,
                                                          float inv_keep, uint32_t k0, uint32_t k1, uint32_t sid,
                                                          const int* __restrict__ step, float* __restrict__ xc,
                                                          float* __restrict__ mask, int* __restrict__ amax) {
  constexpr int LD = EcP + 1, KS = EcP / 4, FP = NCT * 16;
  __shared__ float tab[CVMAX * EcP];
  __shared__ float win[4][18 * LD];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = lane & 15, kq = lane >> 4;
  for (int i = threadIdx.x; i < CV * EcP; i += 256) tab[i] = cemb[i];
  for (int i = lane; i < 18 * LD; i += 64) win[w][i] = 0.f;
  float wres[NCT][3][KS];          // Wc[ct*16 + col][tap][4 s + kq], resident for all of the wave's words
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int tap = 0; tap < 3; ++tap)
#pragma unroll
      for (int s = 0; s < KS; ++s) wres[ct][tap][s] = wc[((ct * 16 + col) * 3 + tap) * EcP + 4 * s + kq];
  const float bias = kq < NCT ? bc[kq * 16 + col] : 0.f;
  const uint32_t st = step ? (uint32_t)step[0] : 0u;
  __syncthreads();
  for (int tok = blockIdx.x * 4 + w; tok < n; tok += gridDim.x * 4) {
    int len;
    const int id = load_ids(chars, tok, lane, len);
    fill_window<EcP>(win[w], tab, id, len, CV, lane);
    wave_sync();
    f32x4 acc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tap = 0; tap < 3; ++tap)
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const float a = win[w][(col + tap) * LD + 4 * s + kq];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
          acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wres[ct][tap][s], acc[ct], 0, 0, 0);
      }
    wave_sync();
    // the lane's rows are kq*4 + i; first index wins a tie at every step
    float best = 0.f;
    int bi = -1;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      float v = -INFINITY;
      int ix = CC;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = kq * 4 + i;
        const float c = row < len ? acc[ct][i] : -INFINITY;
        if (c > v) { v = c; ix = row; }
      }
#pragma unroll
      for (int o = 16; o <= 32; o <<= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(ix, o, 64);
        if (ov > v || (ov == v && oi < ix)) { v = ov; ix = oi; }
      }
      if (ct == kq) { best = v; bi = ix; }
    }
    if (kq < NCT) {   // lane group kq finishes column tile kq
      const long long o = (long long)tok * FP + kq * 16 + col;
      const float feat = len > 0 ? best + bias : 0.f;
      float m = 1.f;
      if (mask) {
        const unsigned long long vec = (unsigned long long)o >> 2;
        const U4 r = philox4x32_10((uint32_t)vec, (uint32_t)(vec >> 32), sid, st, k0, k1);
        const int e = col & 3;
        const uint32_t bits = e == 0 ? r.v[0] : e == 1 ? r.v[1] : e == 2 ? r.v[2] : r.v[3];
        m = u01(bits) >= p ? inv_keep : 0.f;
        mask[o] = m;
      }
      xc[o] = feat * m;
      amax[o] = len > 0 ? bi : -1;
    }
  }
}

template <int EcP, int NCT>
__global__ __launch_bounds__(256) void charcnn_bwd_kernel(const uint8_t* __restrict__ chars,
                                                          const float* __restrict__ cemb, const float* __restrict__ wc,
                                                          const float* __restrict__ dxc, const float* __restrict__ mask,
                                                          const int* __restrict__ amax, int n, int CV,
                                                          float* __restrict__ ws_w, float* __restrict__ ws_t) {
  constexpr int LD = EcP + 1, FP = NCT * 16, ET = EcP / 16, KS = FP / 4, NG = 256 / EcP;
  constexpr int NW = 3 * EcP * FP + FP;
  __shared__ float dtab[CVMAX * EcP];
  __shared__ float win[4][18 * LD];
  __shared__ float stage[4][16 * LD];
  __shared__ float gsh[4][64];
  __shared__ int ash[4][64];
  __shared__ int sids[4][16];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = lane & 15, kq = lane >> 4;
  for (int i = threadIdx.x; i < CV * EcP; i += 256) dtab[i] = 0.f;
  for (int i = lane; i < 18 * LD; i += 64) win[w][i] = 0.f;
  float wres[3][KS][ET];           // Wc[4 s + kq][tap][et*16 + col]: the B operand of dX, K = 3 FP
#pragma unroll
  for (int tap = 0; tap < 3; ++tap)
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int et = 0; et < ET; ++et) wres[tap][s][et] = wc[((4 * s + kq) * 3 + tap) * EcP + et * 16 + col];
  float dw[3][EcP], db = 0.f;      // the lane's filter (lane < FP)
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int e = 0; e < EcP; ++e) dw[k][e] = 0.f;
  __syncthreads();
  const int per = gridDim.x * 4;
  const int rounds = (n + per - 1) / per;
  for (int it = 0; it < rounds; ++it) {
    const int tok = (it * gridDim.x + blockIdx.x) * 4 + w;
    int len = 0, id = 0;
    if (tok < n) id = load_ids(chars, tok, lane, len);
    if (lane < 16) sids[w][lane] = (lane < len && id != 0 && id < CV) ? id : -1;
    if (len > 0) {
      fill_window<EcP>(win[w], cemb, id, len, CV, lane);
      float g = 0.f;
      int a = -1;
      if (lane < FP) {
        const long long o = (long long)tok * FP + lane;
        a = amax[o];
        g = mask ? dxc[o] * mask[o] : dxc[o];
        if ((unsigned)a >= (unsigned)CC) { a = -1; g = 0.f; }
      }
      gsh[w][lane] = g;
      ash[w][lane] = a;
      wave_sync();
      if (a >= 0) {
        db += g;
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
          for (int e = 0; e < EcP; ++e) dw[k][e] += g * win[w][(a + k) * LD + e];
      }
      f32x4 acc[ET];
#pragma unroll
      for (int et = 0; et < ET; ++et) acc[et] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const float gf = gsh[w][4 * s + kq];
        const int af = ash[w][4 * s + kq];
#pragma unroll
        for (int tap = 0; tap < 3; ++tap) {
          const float av = af + tap - 1 == col ? gf : 0.f;   // A_tap[q = col][f = 4 s + kq]
#pragma unroll
          for (int et = 0; et < ET; ++et)
            acc[et] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wres[tap][s][et], acc[et], 0, 0, 0);
        }
      }
#pragma unroll
      for (int et = 0; et < ET; ++et)
#pragma unroll
        for (int i = 0; i < 4; ++i) stage[w][(kq * 4 + i) * LD + et * 16 + col] = acc[et][i];
    }
    __syncthreads();
    {   // thread (e, grp) owns dtab[id][e] of the ids with id % NG == grp and adds their rows in staged order
      const int e = threadIdx.x % EcP, grp = threadIdx.x / EcP;
      for (int ww = 0; ww < 4; ++ww)
        for (int q = 0; q < CC; ++q) {
          const int rid = sids[ww][q];
          if (rid >= 0 && rid % NG == grp) dtab[rid * EcP + e] += stage[ww][q * LD + e];
        }
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < CV * EcP; i += 256) ws_t[(long long)blockIdx.x * CV * EcP + i] = dtab[i];
  // the table's LDS (NW <= 256 EcP floats) now folds the four waves' dWc | dbc, wave 0 to 3 in turn, filter-minor
  for (int ww = 0; ww < 4; ++ww) {
    __syncthreads();
    if (w == ww && lane < FP) {
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int e = 0; e < EcP; ++e) {
          const int o = (k * EcP + e) * FP + lane;
          dtab[o] = ww ? dtab[o] + dw[k][e] : dw[k][e];
        }
      dtab[3 * EcP * FP + lane] = ww ? dtab[3 * EcP * FP + lane] + db : db;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NW; i += 256) ws_w[(long long)blockIdx.x * NW + i] = dtab[i];
}

// dwc [FP][3 EcP] | dbc [FP] | dcemb [CV EcP] = the G partials summed in a fixed order, in fp64 (a sequential fp32 sum of
// up to 128 partials would carry more rounding error than the rest of the backward), rounded once.  A workgroup
// folds 64 consecutive partial elements (coalesced reads); its four waves take a quarter of the partials each, in
// index order, and wave 0 adds the four sums in wave order.
__global__ __launch_bounds__(256) void charcnn_fold_kernel(const float* __restrict__ ws_w, const float* __restrict__ ws_t,
                                                           int G, int EcP, int FP, int CV, float* __restrict__ dwc,
                                                           float* __restrict__ dbc, float* __restrict__ dcemb) {
  __shared__ double red[4][64];
  const int K3 = 3 * EcP, NW = K3 * FP + FP, NT = CV * EcP;
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + lane;
  const int per = (G + 3) / 4, p0 = q * per, p1 = min(G, p0 + per);
  double s = 0.0;
  if (i < NW + NT) {
    const float* src = i < NW ? ws_w + i : ws_t + (i - NW);
    const long long stride = i < NW ? NW : NT;
#pragma unroll 8
    for (int part = p0; part < p1; ++part) s += (double)src[part * stride];
  }
  red[q][lane] = s;
  __syncthreads();
  if (q == 0 && i < NW + NT) {
    const float t = (float)(((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]);
    if (i < K3 * FP) dwc[(i % FP) * K3 + i / FP] = t;     // the partial is filter-minor
    else if (i < NW) dbc[i - K3 * FP] = t;
    else dcemb[i - NW] = t;
  }
}

int charcnn_grid(int n) { return n <= 0 ? 0 : (rk_cdiv(n, 4) < GRID_CAP ? rk_cdiv(n, 4) : GRID_CAP); }
bool charcnn_extents_ok(int EcP, int FP, int CV) {
  return (EcP == 16 || EcP == 32) && FP >= 16 && FP <= 64 && FP % 16 == 0 && CV >= 1 && CV <= CVMAX;
}

}  // namespace

#define RK_CHARCNN_DISPATCH(KERNEL, ...)                                                                       \
  do {                                                                                                         \
    const int key = (EcP == 32 ? 4 : 0) + FP / 16 - 1;                                                         \
    switch (key) {                                                                                             \
      case 0: hipLaunchKernelGGL((KERNEL<16, 1>), dim3(G), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); break; \
      case 1: hipLaunchKernelGGL((KERNEL<16, 2>), dim3(G), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); break; \
      case 2: hipLaunchKernelGGL((KERNEL<16, 3>), dim3(G), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); break; \
      case 3: hipLaunchKernelGGL((KERNEL<16, 4>), dim3(G), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); break; \
      case 4: hipLaunchKernelGGL((KERNEL<32, 1>), dim3(G), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); break; \
      case 5: hipLaunchKernelGGL((KERNEL<32, 2>), dim3(G), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); break; \
      case 6: hipLaunchKernelGGL((KERNEL<32, 3>), dim3(G), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); break; \
      default: hipLaunchKernelGGL((KERNEL<32, 4>), dim3(G), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); break; \
    }                                                                                                          \
  } while (0)

// xc [n][FP] = dropout(bc + max over positions of the width-3 convolution of the gathered characters); mask
// (nullable when p == 0) gets the 0 / (1 / (1 - p)) multipliers, amax the winning positions
extern "C" int rk_charcnn_fwd(const unsigned char* chars, const float* cemb, const float* wc, const float* bc, int n,
                              int EcP, int FP, int CV, float p, unsigned long long seed, int stream_id,
                              const int* step, float* xc, float* mask, int* amax, void* stream) {
  if (n <= 0) return RK_OK;
  if (!charcnn_extents_ok(EcP, FP, CV) || p < 0.f || p >= 1.f) return RK_EBADARG;
  if (p > 0.f && !mask) return RK_EBADARG;
  const int G = charcnn_grid(n);
  float* const mk = p > 0.f ? mask : nullptr;
  RK_CHARCNN_DISPATCH(charcnn_fwd_kernel, chars, cemb, wc, bc, n, CV, p, 1.0f / (1.0f - p), (uint32_t)seed,
                      (uint32_t)(seed >> 32), (uint32_t)stream_id, step, xc, mk, amax);
  RK_LAUNCH_CHECK();
  return RK_OK;
}

// bytes of the backward's workspace
extern "C" long long rk_charcnn_ws_bytes(int n, int EcP, int FP, int CV) {
  if (n <= 0 || !charcnn_extents_ok(EcP, FP, CV)) return 0;
  const long long G = charcnn_grid(n);
  return G * (3ll * EcP * FP + FP + (long long)CV * EcP) * 4;
}

// dwc [FP][3][EcP], dbc [FP], dcemb [CV][EcP] (all fully written) from dxc, the forward's mask (nullable) and amax
extern "C" int rk_charcnn_bwd(const unsigned char* chars, const float* cemb, const float* wc, const float* dxc,
                              const float* mask, const int* amax, int n, int EcP, int FP, int CV, float* dwc,
                              float* dbc, float* dcemb, void* ws, void* stream) {
  if (n <= 0) return RK_OK;
  if (!charcnn_extents_ok(EcP, FP, CV) || !ws) return RK_EBADARG;
  const int G = charcnn_grid(n);
  float* const ws_w = (float*)ws;
  float* const ws_t = ws_w + (long long)G * (3 * EcP * FP + FP);
  RK_CHARCNN_DISPATCH(charcnn_bwd_kernel, chars, cemb, wc, dxc, mask, amax, n, CV, ws_w, ws_t);
  RK_LAUNCH_CHECK();
  const int total = 3 * EcP * FP + FP + CV * EcP;
  hipLaunchKernelGGL(charcnn_fold_kernel, dim3(rk_cdiv(total, 64)), dim3(256), 0, (hipStream_t)stream, ws_w, ws_t, G,
                     EcP, FP, CV, dwc, dbc, dcemb);
  RK_LAUNCH_CHECK();
  return RK_OK;
}
