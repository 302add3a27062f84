// Boundary metrics of a segmentation batch -- HD95, ASSD and NSD (surface Dice) -- on an exact integer squared
// Euclidean distance transform.  An addition over the reference, whose validation only has the confusion-matrix
// metrics (utils/metrics.py:4-13).  Pipeline of one `update` (all on the stream, nothing read back):
//   surf_labels    logits + target -> two uint8 label planes per image (argmax once per pixel; 255 = no class)
//   surf_boundary  label planes -> per (source, n, class) boundary bitmap (4-neighbour erosion, frame = boundary)
//   edt_sq         bitmap -> squared distance to its nearest set pixel: a column scan (one thread per column)
//                  and a row pass min_x' (x - x')^2 + g(x')^2 over the row staged in LDS; in the metric path only
//                  at the boundary pixels of the OTHER source (sel), -1 elsewhere
//   surf_reduce    one block per (direction, n, class): |D|, #{d2 <= T}, sum sqrt(d2) (fp64, fixed order) and the
//                  two order statistics of the q95 rank by bisection on the integer value
//   surf_finalize  empty-mask rules + the per-class state, images added in n order
// All arithmetic up to the square roots is integer, so every count and order statistic is exact and the whole
// result is bitwise repeatable.  The boundary loss takes its signed distance map from the same column + row scheme
// (sdf_* below), straight from the int64 labels.
#include "common.h"
#include "launchers.h"

namespace {
constexpr int kBlock = 256;
constexpr int kColBlock = 64;
constexpr int kRedBlock = 512;
// Vertical "no set pixel in this column": (x - x')^2 + kColNone <= INT32_MAX for |x - x'| < kEdtMaxDim, and every
// real squared distance (<= 2 * kEdtMaxDim^2) is below it.
constexpr int kColNone = kEdtNone - kEdtMaxDim * kEdtMaxDim;
constexpr int kNoLabel = 255;

__global__ __launch_bounds__(kBlock) void surf_labels_kernel(const float* __restrict__ logits,
                                                             const int64_t* __restrict__ target,
                                                             uint8_t* __restrict__ lab, int N, int C, long HW,
                                                             int ignore_index) {
  const long P = (long)N * HW;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < P; i += (long)gridDim.x * kBlock) {
    const long t = target[i];
    int lp = kNoLabel, lt = kNoLabel;
    if (t != ignore_index && t >= 0 && t < C) {
      const long n = i / HW, p = i - n * HW;
      const float* x = logits + n * C * HW + p;
      int best = 0;
      float bv = x[0];
      for (int c = 1; c < C; ++c) {
        const float v = x[c * HW];
        if (v > bv) { bv = v; best = c; }
      }
      lp = best;
      lt = (int)t;
    }
    lab[i] = (uint8_t)lp;
    lab[P + i] = (uint8_t)lt;
  }
}

__global__ __launch_bounds__(kBlock) void surf_boundary_kernel(const uint8_t* __restrict__ lab,
                                                               uint8_t* __restrict__ bnd, long B, int K, int H,
                                                               int W) {
  const long HW = (long)H * W, P = B * HW;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < P; i += (long)gridDim.x * kBlock) {
    const long b = i / HW, p = i - b * HW;
    const int y = (int)(p / W), x = (int)(p - (long)y * W);
    const int L = lab[i];
    bool edge = false;
    if (L >= 1 && L <= K) {
      edge = x == 0 || x == W - 1 || y == 0 || y == H - 1;
      if (!edge) edge = lab[i - 1] != L || lab[i + 1] != L || lab[i - W] != L || lab[i + W] != L;
    }
    uint8_t* o = bnd + b * K * HW + p;
    for (int k = 0; k < K; ++k) o[k * HW] = (uint8_t)(edge && L == k + 1);
  }
}

// One thread per column: downward scan leaves the distance to the nearest set pixel above (or kEdtMaxDim, "none"),
// the upward scan takes the minimum with the one below and stores its square.
__global__ __launch_bounds__(kColBlock) void edt_col_kernel(const uint8_t* __restrict__ mask, int* __restrict__ g2,
                                                            int H, int W) {
  const int x = blockIdx.x * kColBlock + threadIdx.x;
  if (x >= W) return;
  const long base = (long)blockIdx.y * H * W + x;
  const uint8_t* m = mask + base;
  int* g = g2 + base;
  int d = kEdtMaxDim;
  for (int y = 0; y < H; ++y) {
    d = m[(long)y * W] ? 0 : (d < kEdtMaxDim ? d + 1 : kEdtMaxDim);
    g[(long)y * W] = d;
  }
  d = kEdtMaxDim;
  for (int y = H - 1; y >= 0; --y) {
    const int up = g[(long)y * W];
    d = up == 0 ? 0 : (d < kEdtMaxDim ? d + 1 : kEdtMaxDim);
    const int v = up < d ? up : d;
    g[(long)y * W] = v >= kEdtMaxDim ? kColNone : v * v;
  }
}

// One block per (image, row): the row's g^2 is staged in LDS and every evaluated pixel takes the plain minimum
// over the row (branch-free, LDS broadcast reads).  In place: d2 holds g^2 on entry.
__global__ __launch_bounds__(kBlock) void edt_row_kernel(int* __restrict__ d2, const uint8_t* __restrict__ sel,
                                                         long half, long B, int H, int W) {
  extern __shared__ int srow[];
  const long r = blockIdx.x;   // b * H + y
  int* row = d2 + r * W;
  const uint8_t* srw = nullptr;
  if (sel) {
    const long b = r / H, y = r - b * H;
    long ob = b + half;
    if (ob >= B) ob -= B;
    srw = sel + (ob * H + y) * W;
    int any = 0;
    for (int x = threadIdx.x; x < W; x += kBlock) any |= srw[x];
    if (!__syncthreads_or(any)) {
      for (int x = threadIdx.x; x < W; x += kBlock) row[x] = -1;
      return;
    }
  }
  for (int x = threadIdx.x; x < W; x += kBlock) srow[x] = row[x];
  __syncthreads();
  for (int x = threadIdx.x; x < W; x += kBlock) {
    if (srw && !srw[x]) { row[x] = -1; continue; }
    int best = kEdtNone;
    for (int xp = 0; xp < W; ++xp) {
      const int dx = x - xp;
      const int v = dx * dx + srow[xp];
      best = v < best ? v : best;
    }
    row[x] = best >= kColNone ? kEdtNone : best;
  }
}

// block-wide sum of one long per thread (fixed tree); every thread gets the result
__device__ __forceinline__ long block_sum(long v, long* sh) {
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = kRedBlock / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  return sh[0];
}

__device__ __forceinline__ long count_le(const int* v, long n, int thr, long* sh) {
  long c = 0;
  for (long i = threadIdx.x; i < n; i += kRedBlock) c += v[i] <= thr;
  return block_sum(c, sh);
}

// smallest value whose rank range covers k (0-based order statistic) of v[0..n), values in [0, vmax]
__device__ __forceinline__ int kth_value(const int* v, long n, long k, int vmax, long* sh) {
  int lo = 0, hi = vmax;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (count_le(v, n, mid, sh) >= k + 1) hi = mid; else lo = mid + 1;
  }
  return lo;
}

__global__ __launch_bounds__(kRedBlock) void surf_reduce_kernel(int* __restrict__ d2, int64_t* __restrict__ stats,
                                                                double* __restrict__ sums, long HW, int vmax,
                                                                int tol2) {
  __shared__ long sh[kRedBlock];
  __shared__ double shd[kRedBlock];
  __shared__ int fill;
  int* v = d2 + (long)blockIdx.x * HW;
  if (threadIdx.x == 0) fill = 0;
  long cnt = 0, within = 0;
  double sum = 0.0;
  // Members are compacted to the front of the image in place: a chunk is read by every thread before any of its
  // members is written, and write positions (< members so far) never reach past the chunk just read.
  for (long base = 0; base < HW; base += kRedBlock) {
    const long i = base + threadIdx.x;
    const int d = i < HW ? v[i] : -1;
    __syncthreads();
    if (d >= 0) {
      cnt += 1;
      within += d <= tol2;
      sum += sqrt((double)d);
      v[atomicAdd(&fill, 1)] = d;
    }
  }
  const long n = block_sum(cnt, sh);
  const long nin = block_sum(within, sh);
  shd[threadIdx.x] = sum;
  __syncthreads();
  for (int s = kRedBlock / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) shd[threadIdx.x] += shd[threadIdx.x + s];
    __syncthreads();
  }
  long vlo = 0, vhi = 0;
  if (n > 0) {   // block-uniform
    const double pos = 0.95 * (double)(n - 1);
    const long klo = (long)floor(pos), khi = (long)ceil(pos);
    vlo = kth_value(v, n, klo, vmax, sh);
    vhi = vlo;
    if (khi != klo && count_le(v, n, (int)vlo, sh) < khi + 1) vhi = kth_value(v, n, khi, vmax, sh);
  }
  if (threadIdx.x == 0) {
    int64_t* o = stats + (long)blockIdx.x * kSurfStatCols;
    o[0] = n;
    o[1] = nin;
    o[2] = vlo;
    o[3] = vhi;
    sums[blockIdx.x] = shd[0];
  }
}

// numpy / torch.quantile linear interpolation between the two order statistics (torch's lerp form)
__device__ __forceinline__ double q95_of(long n, long vlo, long vhi) {
  const double pos = 0.95 * (double)(n - 1);
  const double w = pos - floor(pos);
  const double a = sqrt((double)vlo), b = sqrt((double)vhi);
  return w < 0.5 ? a + w * (b - a) : b - (b - a) * (1.0 - w);
}

__global__ __launch_bounds__(kBlock) void surf_finalize_kernel(const int64_t* __restrict__ stats,
                                                               const double* __restrict__ sums,
                                                               double* __restrict__ sum, int64_t* __restrict__ count,
                                                               int64_t* __restrict__ onesided,
                                                               double* __restrict__ per_image, int N, int K,
                                                               double diag) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= K) return;
  double s_hd = 0.0, s_as = 0.0, s_ns = 0.0;
  long scored = 0, one = 0;
  const long half = (long)N * K;
  for (int n = 0; n < N; ++n) {
    const long b = (long)n * K + k;
    const int64_t* pg = stats + b * kSurfStatCols;
    const int64_t* gp = stats + (half + b) * kSurfStatCols;
    const long np = pg[0], ng = gp[0];
    double hd = nan(""), as = nan(""), ns = nan("");
    if (np > 0 && ng > 0) {
      const double qa = q95_of(np, pg[2], pg[3]), qb = q95_of(ng, gp[2], gp[3]);
      hd = qa > qb ? qa : qb;
      as = (sums[b] + sums[half + b]) / (double)(np + ng);
      ns = (double)(pg[1] + gp[1]) / (double)(np + ng);
    } else if (np > 0 || ng > 0) {
      hd = diag;
      as = diag;
      ns = 0.0;
      one += 1;
    }
    if (np > 0 || ng > 0) {
      s_hd += hd;
      s_as += as;
      s_ns += ns;
      scored += 1;
    }
    if (per_image) {
      per_image[b * 3 + 0] = hd;
      per_image[b * 3 + 1] = as;
      per_image[b * 3 + 2] = ns;
    }
  }
  sum[k] += s_hd;
  sum[K + k] += s_as;
  sum[2 * K + k] += s_ns;
  count[k] += scored;
  onesided[k] += one;
}

// ---- signed squared distance map of a label batch (boundary loss).  Per (image, class c of the list): pos = valid
// pixels labelled c, neg = the other valid pixels (valid as in the losses: t != ignore_index and 0 <= t < C).
//   sdf_col  one thread per column walks down and up once and leaves BOTH vertical fields packed in the int32
//            output plane: low half = distance to the nearest pos pixel of the column, high half = to the nearest
//            neg pixel (kSdfColNone = no such pixel; extents <= kSdfMaxDim keep real distances far below it)
//   sdf_row  one block per (plane, row) stages the row as interleaved {gpos^2, gneg^2} in LDS (squared while
//            staging) and overwrites it with the result: a pos pixel (gpos == 0) takes -min over the neg field, a
//            neg pixel +min over the pos field, an invalid pixel (neither is 0) scans nothing and gets 0.  A plane
//            without pos or without neg pixels shows in every row (a whole field is "none") and becomes 0.
//            The minimum is the plain branch-free scan of the whole row: an outward scan that stops once
//            d^2 >= best measured 1.3x slower on lesion-like targets (profiles/boundary_loss).
// Integer arithmetic only, no atomics: bitwise repeatable.
constexpr unsigned kSdfColNone = 0xffffu;
constexpr int kSdfNone2 = 1 << 30;   // staged square of "none": dx^2 + kSdfNone2 < 2^31, above every real d^2 (<= 2^23)
constexpr int kSdfRowBlock = 1024;

__global__ __launch_bounds__(kColBlock) void sdf_col_kernel(const int64_t* __restrict__ target,
                                                            int* __restrict__ out, SdfClasses cls, int K, int C,
                                                            int H, int W, int ignore_index, long plane0) {
  const int x = blockIdx.x * kColBlock + threadIdx.x;
  if (x >= W) return;
  const long plane = plane0 + blockIdx.y;   // n * K + k
  const long n = plane / K;
  const int c = cls.c[plane - n * K];
  const int64_t* t = target + n * (long)H * W + x;
  unsigned* g = reinterpret_cast<unsigned*>(out) + plane * (long)H * W + x;
  unsigned dp = kSdfColNone, dn = kSdfColNone;
  for (int y = 0; y < H; ++y) {
    const long v = t[(long)y * W];
    const bool valid = v != ignore_index && v >= 0 && v < C;
    const bool pos = valid && v == c, neg = valid && v != c;
    dp = pos ? 0u : (dp < kSdfColNone ? dp + 1u : kSdfColNone);
    dn = neg ? 0u : (dn < kSdfColNone ? dn + 1u : kSdfColNone);
    g[(long)y * W] = dp | (dn << 16);
  }
  dp = dn = kSdfColNone;
  for (int y = H - 1; y >= 0; --y) {
    const unsigned up = g[(long)y * W];
    const unsigned upp = up & 0xffffu, upn = up >> 16;
    dp = upp == 0u ? 0u : (dp < kSdfColNone ? dp + 1u : kSdfColNone);
    dn = upn == 0u ? 0u : (dn < kSdfColNone ? dn + 1u : kSdfColNone);
    g[(long)y * W] = (upp < dp ? upp : dp) | ((upn < dn ? upn : dn) << 16);
  }
}

__global__ __launch_bounds__(kSdfRowBlock) void sdf_row_kernel(int* __restrict__ out, int W) {
  extern __shared__ int srow[];   // [W][2] = {gpos^2, gneg^2}
  int* row = out + (long)blockIdx.x * W;
  int any_p = 0, any_n = 0;
  for (int x = threadIdx.x; x < W; x += blockDim.x) {
    const unsigned v = (unsigned)row[x];
    const int gp = (int)(v & 0xffffu), gn = (int)(v >> 16);
    any_p |= gp != (int)kSdfColNone;
    any_n |= gn != (int)kSdfColNone;
    srow[2 * x] = gp == (int)kSdfColNone ? kSdfNone2 : gp * gp;
    srow[2 * x + 1] = gn == (int)kSdfColNone ? kSdfNone2 : gn * gn;
  }
  // both barriers are block-uniform and order the staging before the reads below
  const bool live = __syncthreads_or(any_p) != 0;
  const bool live_n = __syncthreads_or(any_n) != 0;
  for (int x = threadIdx.x; x < W; x += blockDim.x) {
    const bool pos = srow[2 * x] == 0, neg = srow[2 * x + 1] == 0;
    int res = 0;
    if (live && live_n && (pos || neg)) {
      const int* f = srow + (pos ? 1 : 0);   // pos pixels scan the neg field and vice versa
      int best = kSdfNone2;
      for (int xp = 0; xp < W; ++xp) {
        const int dx = x - xp;
        const int v = dx * dx + f[2 * xp];
        best = v < best ? v : best;
      }
      res = pos ? -best : best;
    }
    row[x] = res;
  }
}

// phi = sqrt(s), 1 - sqrt(-s), 0: correctly rounded root of an exactly representable integer (|s| <= 2^23);
// sqrtf is the IEEE root here, __fsqrt_rn would be the native approximation
__global__ __launch_bounds__(kBlock) void sdf_phi_kernel(const int* __restrict__ s, float* __restrict__ phi, long n) {
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long)gridDim.x * kBlock) {
    const int v = s[i];
    phi[i] = v > 0 ? sqrtf((float)v) : (v < 0 ? 1.f - sqrtf((float)-v) : 0.f);
  }
}

int grid1d(long n) {
  long b = (n + kBlock - 1) / kBlock;
  return (int)(b > 16384 ? 16384 : (b < 1 ? 1 : b));
}
}  // namespace

void sdf_sq(const int64_t* target, int32_t* s, const SdfClasses& cls, int K, int N, int C, int H, int W,
            int ignore_index, hipStream_t st) {
  const long planes = (long)N * K;
  for (long p0 = 0; p0 < planes; p0 += 65535) {   // grid.y carries the plane in the column pass
    const long np = planes - p0 < 65535 ? planes - p0 : 65535;
    hipLaunchKernelGGL(sdf_col_kernel, dim3((W + kColBlock - 1) / kColBlock, (unsigned)np), dim3(kColBlock), 0, st,
                       target, s, cls, K, C, H, W, ignore_index, p0);
  }
  int block = (W + 63) / 64 * 64;
  if (block > kSdfRowBlock) block = kSdfRowBlock;
  hipLaunchKernelGGL(sdf_row_kernel, dim3((unsigned)(planes * H)), dim3(block), (size_t)W * 2 * sizeof(int), st, s, W);
}

void sdf_phi(const int32_t* s, float* phi, long n, hipStream_t st) {
  hipLaunchKernelGGL(sdf_phi_kernel, dim3(grid1d(n)), dim3(kBlock), 0, st, s, phi, n);
}

void surf_labels(const float* logits, const int64_t* target, uint8_t* lab, int N, int C, long HW, int ignore_index,
                 hipStream_t s) {
  hipLaunchKernelGGL(surf_labels_kernel, dim3(grid1d((long)N * HW)), dim3(kBlock), 0, s, logits, target, lab, N, C, HW,
                     ignore_index);
}

void surf_boundary(const uint8_t* lab, uint8_t* bnd, long B, int K, int H, int W, hipStream_t s) {
  hipLaunchKernelGGL(surf_boundary_kernel, dim3(grid1d(B * H * W)), dim3(kBlock), 0, s, lab, bnd, B, K, H, W);
}

void edt_sq(const uint8_t* mask, int32_t* d2, const uint8_t* sel, long half, long B, int H, int W, hipStream_t s) {
  // grid.y carries the image in the column pass: at most 65535 per launch
  for (long b0 = 0; b0 < B; b0 += 65535) {
    const long nb = B - b0 < 65535 ? B - b0 : 65535;
    hipLaunchKernelGGL(edt_col_kernel, dim3((W + kColBlock - 1) / kColBlock, (unsigned)nb), dim3(kColBlock), 0, s,
                       mask + b0 * H * W, d2 + b0 * H * W, H, W);
  }
  hipLaunchKernelGGL(edt_row_kernel, dim3((unsigned)(B * H)), dim3(kBlock), (size_t)W * sizeof(int), s, d2, sel, half,
                     B, H, W);
}

void surf_reduce(int32_t* d2, int64_t* stats, double* sums, long B, long HW, int vmax, int tol2, hipStream_t s) {
  hipLaunchKernelGGL(surf_reduce_kernel, dim3((unsigned)B), dim3(kRedBlock), 0, s, d2, stats, sums, HW, vmax, tol2);
}

void surf_finalize(const int64_t* stats, const double* sums, double* sum, int64_t* count, int64_t* onesided,
                   double* per_image, int N, int K, int H, int W, hipStream_t s) {
  const double diag = sqrt((double)H * H + (double)W * W);
  hipLaunchKernelGGL(surf_finalize_kernel, dim3((K + kBlock - 1) / kBlock), dim3(kBlock), 0, s, stats, sums, sum,
                     count, onesided, per_image, N, K, diag);
}
