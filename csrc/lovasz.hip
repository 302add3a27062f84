// Lovasz-softmax loss (Berman et al., CVPR 2018) on the segmented radix sort of sort.hip.
// A segment is the whole batch (S = 1, length N * HW) or one image (S = N, length HW); a row is one
// (segment, class) pair.  Classes are processed in chunks of CK (row q = s * CK + (c - c_lo) of the chunk's
// workspace); everything small is indexed by the global row s * C + c.
//   lovasz_keys_kernel    : softmax once per pixel; key e = |y - p_c| (0 at invalid pixels), payload
//                           (pixel index in the segment) << 1 | y
//   [sort_segments: keys descending, ties in ascending pixel index]
//   lovasz_count_kernel   : y bits per tile of the sorted row -> cnt[row][blk]
//   lovasz_rowscan_kernel : exclusive scan of cnt[row][.] (one block per row, carry loop) and G = sum y
//   lovasz_coef_kernel    : F_i from the block offset + ballots, g_i in closed form from the integer counts
//                           (1 / U where y = 1, I / (U (U - 1)) where y = 0; 0 for an absent class), block
//                           partial of sum e_i g_i, and sign(p - y) g_i scattered to pixel order [N][C][HW]
//   lovasz_finalize_kernel: one block; row sums in a fixed order (fp64), presence, class mean, 1 / S, the loss
//                           scalar and scale[row] = 1 / (S * #classes averaged in s) or 0
//   lovasz_grad_kernel    : recomputes the softmax; dx_j = p_j (A_j - sum_c A_c p_c), A_c = gup * scale * coef
// A pixel is valid iff t != ignore_index and 0 <= t < C.  No float atomics, no block waits on another block,
// every loop bound known at launch.
#include "common.h"
#include "launchers.h"

namespace {
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxC = 64;
constexpr int kRounds = 16;
constexpr int kWaveKeys = 64 * kRounds;
constexpr int kTile = kWaves * kWaveKeys;   // sorted elements per block of the count / coefficient passes
constexpr int kFinBlock = 1024;

DEVI bool lovasz_valid(long t, int C, int ignore_index) { return t != ignore_index && t >= 0 && t < C; }

// grid over the N * HW pixels, one pixel per lane
__global__ __launch_bounds__(kBlock) void lovasz_keys_kernel(const float* __restrict__ logits,
                                                             const int64_t* __restrict__ target,
                                                             float* __restrict__ keys, unsigned* __restrict__ pay,
                                                             int N, int C, long HW, int ignore_index, int per_image,
                                                             int c_lo, int CK) {
  const long NP = (long)N * HW;
  const long seg_len = per_image ? HW : NP;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < NP; i += (long)gridDim.x * kBlock) {
    const long n = i / HW, hw = i - n * HW;
    const long t = target[i];
    const bool valid = lovasz_valid(t, C, ignore_index);
    const float* xp = logits + n * C * HW + hw;
    float m = -INFINITY;
    for (int c = 0; c < C; ++c) m = fmaxf(m, xp[c * HW]);
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += __expf(xp[c * HW] - m);
    const float inv = 1.f / se;
    const long s = per_image ? n : 0, pix = per_image ? hw : i;
    for (int k = 0; k < CK; ++k) {
      const int c = c_lo + k;
      const float p = __expf(xp[c * HW] - m) * inv;
      const bool y = valid && c == t;
      const long o = (s * CK + k) * seg_len + pix;
      keys[o] = valid ? fabsf((y ? 1.f : 0.f) - p) : 0.f;
      pay[o] = ((unsigned)pix << 1) | (y ? 1u : 0u);
    }
  }
}

// grid (nblk, Qc)
__global__ __launch_bounds__(kBlock) void lovasz_count_kernel(const unsigned* __restrict__ pay,
                                                              unsigned* __restrict__ cnt, long P, int nblk, int C,
                                                              int c_lo, int CK) {
  __shared__ unsigned ws[kWaves];
  const int q = blockIdx.y, blk = blockIdx.x;
  const int row = (q / CK) * C + c_lo + q % CK;
  const unsigned* pr = pay + (long)q * P;
  const long base = (long)blk * kTile;
  unsigned n = 0;
#pragma unroll 4
  for (int r = 0; r < kTile / kBlock; ++r) {
    const long i = base + r * kBlock + threadIdx.x;
    if (i < P) n += pr[i] & 1u;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned t = 0;
    for (int w = 0; w < kWaves; ++w) t += ws[w];
    cnt[(long)row * nblk + blk] = t;
  }
}

// grid (Qc): exclusive scan of the row's block counts in place, the row's total to gtot
__global__ __launch_bounds__(kBlock) void lovasz_rowscan_kernel(unsigned* __restrict__ cnt,
                                                                unsigned* __restrict__ gtot, int nblk, int C,
                                                                int c_lo, int CK) {
  __shared__ unsigned ws[kWaves];
  const int q = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int row = (q / CK) * C + c_lo + q % CK;
  unsigned* r = cnt + (long)row * nblk;
  unsigned carry = 0;
  for (int base = 0; base < nblk; base += kBlock) {
    const int i = base + threadIdx.x;
    const unsigned v = i < nblk ? r[i] : 0u;
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned u = __shfl_up(inc, o, 64);
      if (lane >= o) inc += u;
    }
    __syncthreads();
    if (lane == 63) ws[wv] = inc;
    __syncthreads();
    unsigned off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const unsigned s = ws[w];
      if (w < wv) off += s;
      tot += s;
    }
    if (i < nblk) r[i] = carry + off + inc - v;
    carry += tot;
  }
  if (threadIdx.x == 0) gtot[row] = carry;
}

// grid (nblk, Qc); wave w owns kWaveKeys consecutive sorted elements of the tile, 64 per round
__global__ __launch_bounds__(kBlock) void lovasz_coef_kernel(const float* __restrict__ keys,
                                                             const unsigned* __restrict__ pay,
                                                             const unsigned* __restrict__ cnt,
                                                             const unsigned* __restrict__ gtot,
                                                             float* __restrict__ part, float* __restrict__ coef,
                                                             long P, int nblk, int C, long HW, int per_image,
                                                             int c_lo, int CK) {
  __shared__ unsigned ws[kWaves];
  __shared__ float fs[kWaves];
  const int q = blockIdx.y, blk = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int s = q / CK, c = c_lo + q % CK, row = s * C + c;
  const float* kr = keys + (long)q * P;
  const unsigned* pr = pay + (long)q * P;
  const long base = (long)blk * kTile + wv * kWaveKeys;
  const unsigned G = gtot[row];

  float e[kRounds];
  unsigned pw[kRounds];
  unsigned long long bal[kRounds];
  unsigned wtot = 0;
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const long i = base + r * 64 + lane;
    const bool valid = i < P;
    e[r] = valid ? kr[i] : 0.f;
    pw[r] = valid ? pr[i] : 0u;
    bal[r] = __ballot(valid && (pw[r] & 1u));
    wtot += (unsigned)__popcll(bal[r]);
  }
  if (lane == 0) ws[wv] = wtot;
  __syncthreads();
  unsigned run = cnt[(long)row * nblk + blk];   // y = 1 before this tile
  for (int w = 0; w < wv; ++w) run += ws[w];

  const unsigned long long le = (2ull << lane) - 1ull;   // lanes 0 .. lane
  float acc = 0.f;
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const long i = base + r * 64 + lane;
    if (i < P) {
      const bool y = pw[r] & 1u;
      const unsigned F = run + (unsigned)__popcll(bal[r] & le);
      const unsigned B = (unsigned)(i + 1) - F, I = G - F, U = G + B;
      float g = 0.f;
      if (G > 0) g = y ? 1.f / (float)U : (U > 1 ? (float)I / ((float)U * (float)(U - 1)) : 0.f);
      acc += e[r] * g;
      const long pix = pw[r] >> 1;
      const long n = per_image ? s : pix / HW, hw = per_image ? pix : pix - n * HW;
      coef[(n * C + c) * HW + hw] = e[r] > 0.f ? (y ? -g : g) : 0.f;   // sign(p - y) g
    }
    run += (unsigned)__popcll(bal[r]);
  }
  acc = wave_sum(acc);
  if (lane == 0) fs[wv] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int w = 0; w < kWaves; ++w) t += fs[w];
    part[(long)row * nblk + blk] = t;
  }
}

// one block.  rowloss [S * C] is workspace; scale [S * C] and loss [1] are the results
__global__ __launch_bounds__(kFinBlock) void lovasz_finalize_kernel(const float* __restrict__ part,
                                                                     const unsigned* __restrict__ gtot,
                                                                     float* __restrict__ rowloss,
                                                                     float* __restrict__ scale,
                                                                     float* __restrict__ loss, int S, int C, int nblk,
                                                                     int c0) {
  __shared__ double red[kFinBlock / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int row = wv; row < S * C; row += kFinBlock / 64) {   // one wave per row, lanes stride over the blocks
    const float* p = part + (long)row * nblk;
    double a = 0.0;
    for (int b = lane; b < nblk; b += 64) a += (double)p[b];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if (lane == 0) rowloss[row] = (float)a;
  }
  __threadfence_block();
  __syncthreads();
  double ls = 0.0;
  for (int s = threadIdx.x; s < S; s += kFinBlock) {
    double sum = 0.0;
    int K = 0;
    for (int c = c0; c < C; ++c)
      if (gtot[s * C + c] > 0) { sum += (double)rowloss[s * C + c]; ++K; }
    const float sc = K > 0 ? (float)(1.0 / ((double)S * (double)K)) : 0.f;
    for (int c = 0; c < C; ++c) scale[s * C + c] = (c >= c0 && gtot[s * C + c] > 0) ? sc : 0.f;
    if (K > 0) ls += sum / (double)K;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ls += __shfl_xor(ls, o, 64);
  if (lane == 0) red[wv] = ls;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < kFinBlock / 64; ++w) t += red[w];
    loss[0] = (float)(t / (double)S);
  }
}

// grid over the N * HW pixels, one pixel per lane
__global__ __launch_bounds__(kBlock) void lovasz_grad_kernel(const float* __restrict__ logits,
                                                             const int64_t* __restrict__ target,
                                                             const float* __restrict__ coef,
                                                             const float* __restrict__ scale,
                                                             const float* __restrict__ gup, float* __restrict__ grad,
                                                             int N, int C, long HW, int ignore_index,
                                                             int per_image) {
  const long NP = (long)N * HW;
  const float g0 = gup[0];
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < NP; i += (long)gridDim.x * kBlock) {
    const long n = i / HW, hw = i - n * HW;
    const long o = n * C * HW + hw;
    float* gp = grad + o;
    if (!lovasz_valid(target[i], C, ignore_index)) {
      for (int c = 0; c < C; ++c) gp[c * HW] = 0.f;
      continue;
    }
    const float* xp = logits + o;
    const float* ap = coef + o;
    const float* sc = scale + (per_image ? n * C : 0);
    float m = -INFINITY;
    for (int c = 0; c < C; ++c) m = fmaxf(m, xp[c * HW]);
    float se = 0.f, dot = 0.f;
    for (int c = 0; c < C; ++c) {
      const float ex = __expf(xp[c * HW] - m);
      se += ex;
      dot += ap[c * HW] * sc[c] * ex;
    }
    const float inv = 1.f / se;
    dot *= inv;
    for (int c = 0; c < C; ++c) {
      const float p = __expf(xp[c * HW] - m) * inv;
      gp[c * HW] = g0 * (p * (ap[c * HW] * sc[c] - dot));
    }
  }
}

int grid_for(long n) {
  const long b = (n + kBlock - 1) / kBlock;
  return (int)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}
}  // namespace

int lovasz_max_classes() { return kMaxC; }
int lovasz_tile() { return kTile; }

void lovasz_keys(const float* logits, const int64_t* target, float* keys, unsigned* pay, int N, int C, long HW,
                 int ignore_index, int per_image, int c_lo, int CK, hipStream_t s) {
  lovasz_keys_kernel<<<grid_for((long)N * HW), kBlock, 0, s>>>(logits, target, keys, pay, N, C, HW, ignore_index,
                                                                per_image, c_lo, CK);
}

void lovasz_coef(const float* keys, const unsigned* pay, unsigned* cnt, unsigned* gtot, float* part, float* coef,
                 int N, int C, long HW, int per_image, int c_lo, int CK, hipStream_t s) {
  const int S = per_image ? N : 1;
  const long P = per_image ? HW : (long)N * HW;
  const int nblk = cdiv(P, kTile), Qc = S * CK;
  lovasz_count_kernel<<<dim3(nblk, Qc), kBlock, 0, s>>>(pay, cnt, P, nblk, C, c_lo, CK);
  lovasz_rowscan_kernel<<<Qc, kBlock, 0, s>>>(cnt, gtot, nblk, C, c_lo, CK);
  lovasz_coef_kernel<<<dim3(nblk, Qc), kBlock, 0, s>>>(keys, pay, cnt, gtot, part, coef, P, nblk, C, HW, per_image,
                                                       c_lo, CK);
}

void lovasz_finalize(const float* part, const unsigned* gtot, float* rowloss, float* scale, float* loss, int N, int C,
                     long HW, int per_image, int c0, hipStream_t s) {
  const int S = per_image ? N : 1;
  const long P = per_image ? HW : (long)N * HW;
  lovasz_finalize_kernel<<<1, kFinBlock, 0, s>>>(part, gtot, rowloss, scale, loss, S, C, cdiv(P, kTile), c0);
}

void lovasz_grad(const float* logits, const int64_t* target, const float* coef, const float* scale, const float* gup,
                 float* grad, int N, int C, long HW, int ignore_index, int per_image, hipStream_t s) {
  lovasz_grad_kernel<<<grid_for((long)N * HW), kBlock, 0, s>>>(logits, target, coef, scale, gup, grad, N, C, HW,
                                                                ignore_index, per_image);
}
