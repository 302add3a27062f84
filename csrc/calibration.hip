// Calibration of the softmax output: reliability statistics (ECE / MCE / NLL / Brier), the NLL of a grid of
// inverse temperatures (post-hoc temperature scaling) and per-pixel uncertainty maps.  An addition over the
// reference, which never looks at the probabilities.  ops/calibration.py has the semantics.
//   calib_stats_kernel    : softmax at temperature T in registers, one pass over the classes (running max, the sums
//                           rescaled when it moves).  Per block: an LDS histogram of the two integer tables (bin
//                           count, bin hits; one row per wave), flushed with integer atomics as confmat_kernel does,
//                           and ONE fp64 partial per floating sum -- row [M + 2] = conf_sum[M], nll_sum, brier_sum of
//                           part.  A wave visits each distinct bin among its 64 pixels once: two ballots count the
//                           pixels and the hits, one masked butterfly sums the confidences.
//   calib_nll_grid_kernel : pass 1 max over the classes, pass 2 K log-sum-exps per pixel (K accumulators in
//                           registers: KMAX is a template parameter, the smallest instance >= K runs); row [K] of part.
//   calib_finalize_kernel : one block; column c adds part[0..nb)[c] in block order onto state[c] (wave w takes the
//                           w-th sixteenth of the rows in order, then the sixteen segment sums are added in order).
//   uncertainty_kernel    : four consecutive pixels per thread, one 32-bit store of the four grey levels; float4
//                           loads when a plane is a multiple of four pixels; the last P % 4 pixels store bytes.
// A pixel is valid iff t != ignore_index and 0 <= t < C.  No float atomics, no block waits on another block, the
// grid is a function of the pixel count alone and every reduction has a fixed order: a repeated call gives the
// same bits.
#include "common.h"
#include "launchers.h"

namespace {
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kPixPerBlock = kBlock * 8;
constexpr int kMaxBlocks = 2048;
constexpr int kFinBlock = 1024;
constexpr int kFinWaves = kFinBlock / 64;
constexpr int kFinCols = kCalibMaxBins + 2;   // the widest partial row
static_assert(kCalibMaxK <= kFinCols, "a row of grid sums must fit the finalize table");

DEVI bool calib_valid(long t, int C, int ignore_index) { return t != ignore_index && t >= 0 && t < C; }

DEVI double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(kBlock) void calib_stats_kernel(const float* __restrict__ logits,
                                                             const int64_t* __restrict__ target,
                                                             int64_t* __restrict__ ints, double* __restrict__ part,
                                                             int N, int C, long HW, int ignore_index, int M, float T) {
  __shared__ unsigned wcnt[kWaves][kCalibMaxBins], whit[kWaves][kCalibMaxBins];
  __shared__ double wconf[kWaves][kCalibMaxBins];
  __shared__ double wred[kWaves][2];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int i = tid; i < kWaves * kCalibMaxBins; i += kBlock) {
    (&wcnt[0][0])[i] = 0;
    (&whit[0][0])[i] = 0;
    (&wconf[0][0])[i] = 0.0;
  }
  __syncthreads();
  const long P = (long)N * HW;
  const float fm = (float)M;
  double nll = 0.0, brier = 0.0;
  // the trip count is the same for every thread of the block: the ballots below see whole waves
  for (long base = (long)blockIdx.x * kBlock; base < P; base += (long)gridDim.x * kBlock) {
    const long i = base + tid;
    bool ok = false, hit = false;
    int bin = 0;
    float conf = 0.f;
    if (i < P) {
      const long t = target[i];
      if (calib_valid(t, C, ignore_index)) {
        ok = true;
        const long n = i / HW, p = i - n * HW;
        const float* x = logits + n * C * HW + p;
        float m = x[0] / T, zt = m, s = 1.f, q = 1.f;   // s = sum e^(z - m), q = sum e^(2 (z - m))
        int best = 0;
        for (int c = 1; c < C; ++c) {
          const float v = x[c * HW] / T;
          if (c == t) zt = v;
          if (v > m) {
            const float r = expf(m - v);
            s = fmaf(s, r, 1.f);
            q = fmaf(q, r * r, 1.f);
            m = v;
            best = c;
          } else {
            const float e = expf(v - m);
            s += e;
            q = fmaf(e, e, q);
          }
        }
        conf = 1.f / s;
        const float pt = expf(zt - m) * conf;
        nll += (double)(logf(s) + (m - zt));
        brier += (double)(q * conf * conf - 2.f * pt + 1.f);
        bin = max(0, min(M - 1, (int)(conf * fm)));
        hit = best == t;
      }
    }
    unsigned long long todo = __ballot(ok);
    while (todo) {
      const int lb = __shfl(bin, __ffsll((long long)todo) - 1, 64);
      const bool mine = ok && bin == lb;
      const unsigned long long members = __ballot(mine), hits = __ballot(mine && hit);
      const double sum = wave_sum_d(mine ? (double)conf : 0.0);
      if (lane == 0) {      // this wave's row: no other lane or wave writes it
        wcnt[wv][lb] += (unsigned)__popcll(members);
        whit[wv][lb] += (unsigned)__popcll(hits);
        wconf[wv][lb] += sum;
      }
      todo &= ~members;
    }
  }
  nll = wave_sum_d(nll);
  brier = wave_sum_d(brier);
  if (lane == 0) {
    wred[wv][0] = nll;
    wred[wv][1] = brier;
  }
  __syncthreads();
  double* row = part + (long)blockIdx.x * (M + 2);
  for (int b = tid; b < M; b += kBlock) {
    double a = 0.0;
    unsigned long long cnt = 0, hits = 0;
    for (int w = 0; w < kWaves; ++w) {
      a += wconf[w][b];
      cnt += wcnt[w][b];
      hits += whit[w][b];
    }
    row[b] = a;
    if (cnt) atomicAdd(reinterpret_cast<unsigned long long*>(ints + b), cnt);
    if (hits) atomicAdd(reinterpret_cast<unsigned long long*>(ints + M + b), hits);
  }
  if (tid == 0) {
    double a = 0.0, b = 0.0;
    for (int w = 0; w < kWaves; ++w) {
      a += wred[w][0];
      b += wred[w][1];
    }
    row[M] = a;
    row[M + 1] = b;
  }
}

// betas holds kCalibMaxK floats (the caller pads): every unrolled read is in bounds
template <int KMAX>
__global__ __launch_bounds__(kBlock) void calib_nll_grid_kernel(const float* __restrict__ logits,
                                                                const int64_t* __restrict__ target,
                                                                const float* __restrict__ betas,
                                                                double* __restrict__ part, int N, int C, long HW,
                                                                int ignore_index, int K) {
  __shared__ double wred[kWaves][KMAX];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float beta[KMAX];
  double ts[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    beta[k] = betas[k];
    ts[k] = 0.0;
  }
  const long P = (long)N * HW;
  for (long i = (long)blockIdx.x * kBlock + tid; i < P; i += (long)gridDim.x * kBlock) {
    const long t = target[i];
    if (!calib_valid(t, C, ignore_index)) continue;
    const long n = i / HW, p = i - n * HW;
    const float* x = logits + n * C * HW + p;
    float m = x[0];
    for (int c = 1; c < C; ++c) m = fmaxf(m, x[c * HW]);
    const float gap = m - x[t * HW];
    float acc[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) acc[k] = 0.f;
    for (int c = 0; c < C; ++c) {
      const float d = x[c * HW] - m;
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) acc[k] += __expf(beta[k] * d);
    }
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) ts[k] += (double)(logf(acc[k]) + beta[k] * gap);
  }
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    if (k < K) {
      const double v = wave_sum_d(ts[k]);
      if (lane == 0) wred[wv][k] = v;
    }
  }
  __syncthreads();
  if (tid < K) {
    double a = 0.0;
    for (int w = 0; w < kWaves; ++w) a += wred[w][tid];
    part[(long)blockIdx.x * K + tid] = a;
  }
}

__global__ __launch_bounds__(kFinBlock) void calib_finalize_kernel(const double* __restrict__ part,
                                                                   double* __restrict__ state, int nb, int cols) {
  __shared__ double seg[kFinWaves][kFinCols];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int per = (nb + kFinWaves - 1) / kFinWaves;
  const int b0 = min(wv * per, nb), b1 = min(b0 + per, nb);
  for (int c = lane; c < cols; c += 64) {
    double a = 0.0;
    int b = b0;
    for (; b + 8 <= b1; b += 8) {   // eight loads in flight, added in row order
      double v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = part[(long)(b + i) * cols + c];
#pragma unroll
      for (int i = 0; i < 8; ++i) a += v[i];
    }
    for (; b < b1; ++b) a += part[(long)b * cols + c];
    seg[wv][c] = a;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < cols; c += kFinBlock) {
    double a = 0.0;
    for (int w = 0; w < kFinWaves; ++w) a += seg[w][c];
    state[c] += a;
  }
}

// grey level of one pixel from its max-shifted sums: s = sum e^d, u = sum e^d d  (d = z / T - max <= 0)
DEVI unsigned unc_level(float s, float u, int mode, float scale) {
  const float v = mode == 0 ? logf(s) - u / s : 1.f - 1.f / s;
  return (unsigned)fminf(fmaxf(rintf(v * scale), 0.f), 255.f);
}

__global__ __launch_bounds__(kBlock) void uncertainty_kernel(const float* __restrict__ logits,
                                                             uint8_t* __restrict__ out, int N, int C, long HW,
                                                             float T, int mode, float scale, int vec_load,
                                                             int vec_store) {
  const long P = (long)N * HW;
  const long i0 = ((long)blockIdx.x * kBlock + threadIdx.x) * 4;
  if (i0 >= P) return;
  float m[4], s[4] = {0.f, 0.f, 0.f, 0.f}, u[4] = {0.f, 0.f, 0.f, 0.f};
  unsigned lev[4];
  const bool full = i0 + 4 <= P;
  if (full && vec_load) {   // the four pixels lie in one image and every class row is 16-byte aligned
    const long n = i0 / HW, p = i0 - n * HW;
    const float* x = logits + n * C * HW + p;
    const float4 v0 = *reinterpret_cast<const float4*>(x);
    m[0] = v0.x / T; m[1] = v0.y / T; m[2] = v0.z / T; m[3] = v0.w / T;
    if (C == 1) {
#pragma unroll
      for (int j = 0; j < 4; ++j) m[j] = fmaxf(m[j], 0.f);
    }
    for (int c = 1; c < C; ++c) {
      const float4 v = *reinterpret_cast<const float4*>(x + c * HW);
      m[0] = fmaxf(m[0], v.x / T); m[1] = fmaxf(m[1], v.y / T);
      m[2] = fmaxf(m[2], v.z / T); m[3] = fmaxf(m[3], v.w / T);
    }
    for (int c = 0; c < C; ++c) {
      const float4 v = *reinterpret_cast<const float4*>(x + c * HW);
      const float z[4] = {v.x / T, v.y / T, v.z / T, v.w / T};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d = z[j] - m[j], e = expf(d);
        s[j] += e;
        u[j] = fmaf(e, d, u[j]);
      }
    }
    if (C == 1) {   // the implicit class-0 logit 0 of a sigmoid head
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d = -m[j], e = expf(d);
        s[j] += e;
        u[j] = fmaf(e, d, u[j]);
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long i = i0 + j;
      if (i >= P) { s[j] = 1.f; continue; }
      const long n = i / HW, p = i - n * HW;
      const float* x = logits + n * C * HW + p;
      float mm = C == 1 ? fmaxf(x[0] / T, 0.f) : x[0] / T;
      for (int c = 1; c < C; ++c) mm = fmaxf(mm, x[c * HW] / T);
      for (int c = 0; c < C; ++c) {
        const float d = x[c * HW] / T - mm, e = expf(d);
        s[j] += e;
        u[j] = fmaf(e, d, u[j]);
      }
      if (C == 1) {
        const float d = -mm, e = expf(d);
        s[j] += e;
        u[j] = fmaf(e, d, u[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) lev[j] = unc_level(s[j], u[j], mode, scale);
  if (full && vec_store) {
    *reinterpret_cast<uint32_t*>(out + i0) = lev[0] | (lev[1] << 8) | (lev[2] << 16) | (lev[3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i0 + j < P) out[i0 + j] = (uint8_t)lev[j];
  }
}
}  // namespace

int calib_blocks(long pixels) {
  const long b = (pixels + kPixPerBlock - 1) / kPixPerBlock;
  return (int)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}

void calib_stats(const float* logits, const int64_t* target, int64_t* ints, double* sums, double* part, int N, int C,
                 long HW, int ignore_index, int M, float T, hipStream_t s) {
  const int nb = calib_blocks((long)N * HW);
  calib_stats_kernel<<<nb, kBlock, 0, s>>>(logits, target, ints, part, N, C, HW, ignore_index, M, T);
  calib_finalize_kernel<<<1, kFinBlock, 0, s>>>(part, sums, nb, M + 2);
}

void calib_nll_grid(const float* logits, const int64_t* target, const float* betas, double* sums, double* part, int N,
                    int C, long HW, int ignore_index, int K, hipStream_t s) {
  const int nb = calib_blocks((long)N * HW);
  if (K <= 8)
    calib_nll_grid_kernel<8><<<nb, kBlock, 0, s>>>(logits, target, betas, part, N, C, HW, ignore_index, K);
  else if (K <= 40)
    calib_nll_grid_kernel<40><<<nb, kBlock, 0, s>>>(logits, target, betas, part, N, C, HW, ignore_index, K);
  else
    calib_nll_grid_kernel<kCalibMaxK><<<nb, kBlock, 0, s>>>(logits, target, betas, part, N, C, HW, ignore_index, K);
  calib_finalize_kernel<<<1, kFinBlock, 0, s>>>(part, sums, nb, K);
}

void uncertainty_map(const float* logits, uint8_t* out, int N, int C, long HW, float T, int mode, hipStream_t s) {
  const long P = (long)N * HW;
  const int ce = C == 1 ? 2 : C;
  const float scale = mode == 0 ? 255.f / logf((float)ce) : 255.f / (1.f - 1.f / (float)ce);
  const int vec_load = (HW % 4 == 0) && (reinterpret_cast<uintptr_t>(logits) % 16 == 0);
  const int vec_store = reinterpret_cast<uintptr_t>(out) % 4 == 0;
  const long blocks = (P + 4L * kBlock - 1) / (4L * kBlock);
  uncertainty_kernel<<<(unsigned)blocks, kBlock, 0, s>>>(logits, out, N, C, HW, T, mode, scale, vec_load, vec_store);
}
