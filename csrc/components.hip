// Connected-component labelling of a batch of uint8 label maps, the per-component integers on top of it, and the
// two consumers: mask clean-up at prediction time (fill holes / remove small objects / keep the largest component)
// and the lesion-wise detection counters.  An addition over the reference, which saves the raw argmax
// (core/seg_trainer.py:162) and only scores overlap (utils/metrics.py:4-13).
//
// Labelling of lab [B][H][W] (a pixel equal to kCcSkip belongs to nothing; any other pixel is connected to a
// 4- or 8-neighbour holding the SAME value, so one launch sequence labels every class, background included):
//   cc_tile     one 256-thread block per 32 x 32 tile: label bytes in LDS, a tile-local union-find in LDS
//               (atomicMin merges, then a flatten), tile-local area / weight sums by LDS atomics; writes the global
//               index of every pixel's tile-local root, and the two sums at the tile-local root's position
//   cc_seam     one thread per pixel of every tile's first row / first column: unites it with its neighbours in
//               the tile above / to the left (and the diagonal ones at connectivity 8) in global memory
//   cc_flatten  root[i] = find(i); a tile-local root that is not the component's root adds its sums to the latter
// parent[i] <= i holds everywhere and always, so find() terminates and the surviving root is the raster-first
// pixel of the component.  Only integer atomicMin / atomicAdd / atomicMax are used: the result does not depend on
// arrival order and is bitwise repeatable.
//
// Every data-dependent loop (find, the retry of a union, the scan loops are plain counted loops) is capped at H*W
// steps, which a correct run cannot reach; hitting the cap counts one error in `err` and leaves the loop, so a bug
// ends as a wrong answer with a nonzero error counter, never as a spinning kernel.  In cc_seam / cc_flatten the
// parent plane is read with agent-scope relaxed atomic loads and written only by agent-scope atomics; everything
// else that crosses workgroups crosses a kernel boundary.
#include "common.h"
#include "launchers.h"

namespace {
constexpr int kBlock = 256;
constexpr int kTile = 32;                    // tile edge
constexpr int kTilePix = kTile * kTile;      // 1024 pixels, 4 per thread
constexpr int kPerThread = kTilePix / kBlock;
constexpr int kSkip = kCcSkip;

#define CC_AGENT __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ int ld_agent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, CC_AGENT); }

// ---- tile-local union-find in LDS --------------------------------------------------------------------------
__device__ __forceinline__ int lds_find(volatile int* par, int i, int cap, int* err) {
  for (int n = 0;; ++n) {
    const int p = par[i];
    if (p == i) return i;
    if (n >= cap || p < 0 || p > i) { atomicAdd(err, 1); return i; }
    i = p;
  }
}

__device__ __forceinline__ void lds_union(int* par, int a, int b, int cap, int* err) {
  for (int n = 0;; ++n) {
    a = lds_find(par, a, cap, err);
    b = lds_find(par, b, cap, err);
    if (a == b) return;
    if (n >= cap) { atomicAdd(err, 1); return; }
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&par[a], b);   // a > b: parent[a] only ever decreases
    if (old == a) return;                    // a was a root and now hangs below b
    a = old;                                 // a had a parent `old` already: unite that one with b
  }
}

// mode 0: weight = pixel on the image frame; mode 1: weight = the other source (plane (b + half) % B) holds the
// same label at this pixel
__global__ __launch_bounds__(kBlock) void cc_tile_kernel(const uint8_t* __restrict__ lab, int* __restrict__ root,
                                                         int* __restrict__ area, int* __restrict__ aux,
                                                         int* __restrict__ err, long half, long B, int H, int W,
                                                         int tilesX, int tilesY, int conn8, int mode, int cap) {
  __shared__ int s_par[kTilePix];
  __shared__ int s_cnt[kTilePix];
  __shared__ int s_aux[kTilePix];
  __shared__ uint8_t s_lab[kTilePix];
  const long tile = blockIdx.x;
  const long perPlane = (long)tilesX * tilesY;
  const long b = tile / perPlane;
  const int t = (int)(tile - b * perPlane);
  const int ty = t / tilesX, tx = t - ty * tilesX;
  const int y0 = ty * kTile, x0 = tx * kTile;
  const long HW = (long)H * W;
  const uint8_t* L = lab + b * HW;
  long ob = b + half;
  if (ob >= B) ob -= B;
  const uint8_t* O = lab + ob * HW;

  int wgt[kPerThread];
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const int p = threadIdx.x + j * kBlock;
    const int ly = p / kTile, lx = p - ly * kTile;
    const int y = y0 + ly, x = x0 + lx;
    int v = kSkip;
    wgt[j] = 0;
    if (y < H && x < W) {
      const long g = (long)y * W + x;
      v = L[g];
      wgt[j] = mode == 0 ? (int)(y == 0 || x == 0 || y == H - 1 || x == W - 1) : (int)(O[g] == v);
    }
    s_lab[p] = (uint8_t)v;
    s_par[p] = v != kSkip ? p : -1;
    s_cnt[p] = 0;
    s_aux[p] = 0;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const int p = threadIdx.x + j * kBlock;
    const int ly = p / kTile, lx = p - ly * kTile;
    const int v = s_lab[p];
    if (v == kSkip) continue;
    if (lx > 0 && s_lab[p - 1] == v) lds_union(s_par, p, p - 1, cap, err);
    if (ly > 0 && s_lab[p - kTile] == v) lds_union(s_par, p, p - kTile, cap, err);
    if (conn8 && ly > 0) {
      if (lx > 0 && s_lab[p - kTile - 1] == v) lds_union(s_par, p, p - kTile - 1, cap, err);
      if (lx < kTile - 1 && s_lab[p - kTile + 1] == v) lds_union(s_par, p, p - kTile + 1, cap, err);
    }
  }
  __syncthreads();
  int r[kPerThread];
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const int p = threadIdx.x + j * kBlock;
    r[j] = -1;
    if (s_lab[p] == kSkip) continue;
    r[j] = lds_find(s_par, p, cap, err);
    atomicAdd(&s_cnt[r[j]], 1);
    if (wgt[j]) atomicAdd(&s_aux[r[j]], wgt[j]);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const int p = threadIdx.x + j * kBlock;
    const int ly = p / kTile, lx = p - ly * kTile;
    const int y = y0 + ly, x = x0 + lx;
    if (y >= H || x >= W) continue;
    const long g = b * HW + (long)y * W + x;
    int gr = -1;
    if (r[j] >= 0) {
      const int ry = r[j] / kTile, rx = r[j] - ry * kTile;
      gr = (y0 + ry) * W + x0 + rx;
    }
    const bool is_root = r[j] == p;
    root[g] = gr;
    area[g] = is_root ? s_cnt[p] : 0;
    aux[g] = is_root ? s_aux[p] : 0;
  }
}

// ---- global union-find on one plane of `root` --------------------------------------------------------------
__device__ __forceinline__ int g_find(const int* par, int i, int cap, int* err) {
  for (int n = 0;; ++n) {
    const int p = ld_agent(par + i);
    if (p == i) return i;
    if (n >= cap || p < 0 || p > i) { atomicAdd(err, 1); return i; }
    i = p;
  }
}

__device__ __forceinline__ void g_union(int* par, int a, int b, int cap, int* err) {
  for (int n = 0;; ++n) {
    a = g_find(par, a, cap, err);
    b = g_find(par, b, cap, err);
    if (a == b) return;
    if (n >= cap) { atomicAdd(err, 1); return; }
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(par + a, b, __ATOMIC_RELAXED, CC_AGENT);
    if (old == a) return;
    a = old;
  }
}

// Threads [0, nSR * W) of a plane: pixel (x, y = (j + 1) * kTile) of a tile's first row, united with the pixel above
// (and above-left / above-right at connectivity 8).  Threads after them: pixel (x = (j + 1) * kTile, y) of a tile's
// first column, united with the pixel to its left (and above-left / below-left).  Every 4- or 8-adjacent pair in
// two different tiles is visited at least once; a pair visited twice is united twice, which changes nothing.
__global__ __launch_bounds__(kBlock) void cc_seam_kernel(const uint8_t* __restrict__ lab, int* __restrict__ root,
                                                         int* __restrict__ err, long B, int H, int W, int nSR, int nSC,
                                                         int conn8, int cap) {
  const long HW = (long)H * W;
  const long nH = (long)nSR * W, per = nH + (long)nSC * H, total = B * per;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long)gridDim.x * kBlock) {
    const long b = i / per;
    const long k = i - b * per;
    const uint8_t* L = lab + b * HW;
    int* par = root + b * HW;
    int x, y;
    if (k < nH) {
      const int j = (int)(k / W);
      x = (int)(k - (long)j * W);
      y = (j + 1) * kTile;
      const int me = y * W + x;
      const int v = L[me];
      if (v == kSkip) continue;
      if (L[me - W] == v) g_union(par, me, me - W, cap, err);
      if (conn8) {
        if (x > 0 && L[me - W - 1] == v) g_union(par, me, me - W - 1, cap, err);
        if (x < W - 1 && L[me - W + 1] == v) g_union(par, me, me - W + 1, cap, err);
      }
    } else {
      const long k2 = k - nH;
      const int j = (int)(k2 / H);
      y = (int)(k2 - (long)j * H);
      x = (j + 1) * kTile;
      const int me = y * W + x;
      const int v = L[me];
      if (v == kSkip) continue;
      if (L[me - 1] == v) g_union(par, me, me - 1, cap, err);
      if (conn8) {
        if (y > 0 && L[me - W - 1] == v) g_union(par, me, me - W - 1, cap, err);
        if (y < H - 1 && L[me + W - 1] == v) g_union(par, me + W - 1, me, cap, err);
      }
    }
  }
}

// root[i] = find(i).  A concurrent store only replaces a parent by one of its ancestors, so every value a find
// can read leads to the same root.  area / aux of a tile-local root that is not the component's root move to the
// latter; nobody else touches such an entry in this launch, and the component's root is only added to.
__global__ __launch_bounds__(kBlock) void cc_flatten_kernel(int* __restrict__ root, int* __restrict__ area,
                                                            int* __restrict__ aux, int* __restrict__ err, long B,
                                                            long HW, int cap) {
  const long P = B * HW;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < P; i += (long)gridDim.x * kBlock) {
    const long b = i / HW;
    const int p = (int)(i - b * HW);
    int* par = root + b * HW;
    if (ld_agent(par + p) < 0) continue;
    const int r = g_find(par, p, cap, err);
    if (r == p) continue;
    __hip_atomic_store(par + p, r, __ATOMIC_RELAXED, CC_AGENT);
    const int a = area[i];
    if (a > 0) {
      atomicAdd(area + b * HW + r, a);
      const int w = aux[i];
      if (w) atomicAdd(aux + b * HW + r, w);
    }
  }
}

// ---- compaction: roots numbered 1..K per plane in raster order (scipy.ndimage.label's numbering) ------------
constexpr int kScanPer = 8;   // consecutive pixels per thread and round
__global__ __launch_bounds__(kBlock) void cc_rank_kernel(const int* __restrict__ root, int* __restrict__ rank,
                                                         int64_t* __restrict__ num, long HW) {
  __shared__ int s[kBlock];
  const int* R = root + (long)blockIdx.x * HW;
  int* K = rank + (long)blockIdx.x * HW;
  long carry = 0;
  for (long base = 0; base < HW; base += (long)kBlock * kScanPer) {
    const long i0 = base + (long)threadIdx.x * kScanPer;
    int mine = 0;
#pragma unroll
    for (int j = 0; j < kScanPer; ++j) mine += (i0 + j < HW && R[i0 + j] == (int)(i0 + j));
    s[threadIdx.x] = mine;
    __syncthreads();
    for (int d = 1; d < kBlock; d <<= 1) {   // inclusive Hillis-Steele scan
      const int v = (int)threadIdx.x >= d ? s[threadIdx.x - d] : 0;
      __syncthreads();
      s[threadIdx.x] += v;
      __syncthreads();
    }
    long at = carry + s[threadIdx.x] - mine;
#pragma unroll
    for (int j = 0; j < kScanPer; ++j)
      if (i0 + j < HW && R[i0 + j] == (int)(i0 + j)) K[i0 + j] = (int)(++at);
    carry += s[kBlock - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) num[blockIdx.x] = carry;
}

// out[i] = src[root[i]] (0 at skipped pixels)
__global__ __launch_bounds__(kBlock) void cc_gather_kernel(const int* __restrict__ root, const int* __restrict__ src,
                                                           int* __restrict__ out, long B, long HW) {
  const long P = B * HW;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < P; i += (long)gridDim.x * kBlock) {
    const long b = i / HW;
    const int r = root[i];
    out[i] = r < 0 ? 0 : src[b * HW + r];
  }
}

// ---- clean-up ------------------------------------------------------------------------------------------------
// key[b][class] = max over the class's components of area << 32 | ~root: largest area, ties to the raster-first
__global__ __launch_bounds__(kBlock) void cc_largest_kernel(const uint8_t* __restrict__ lab,
                                                            const int* __restrict__ root,
                                                            const int* __restrict__ area,
                                                            unsigned long long* __restrict__ key, long B, long HW) {
  const long P = B * HW;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < P; i += (long)gridDim.x * kBlock) {
    const long b = i / HW;
    const int p = (int)(i - b * HW);
    const int v = lab[i];
    if (v == 0 || v == kSkip || root[i] != p) continue;
    const unsigned long long k = ((unsigned long long)(unsigned)area[i] << 32) | (unsigned)~(unsigned)p;
    atomicMax(key + b * kCcKeyCols + v, k);
  }
}

// mode 0 (fill holes; the labelling was 4-connected with the frame weights): a label-0 pixel whose component has
// no frame pixel takes the label left of the component's raster-first pixel.
// mode 1 (prune): a foreground pixel goes to 0 when its component is smaller than min_area or, with `key`, is not
// the class's largest.
__global__ __launch_bounds__(kBlock) void cc_apply_kernel(const uint8_t* __restrict__ lab,
                                                          const int* __restrict__ root,
                                                          const int* __restrict__ area, const int* __restrict__ aux,
                                                          const unsigned long long* __restrict__ key,
                                                          uint8_t* __restrict__ out, long B, long HW, int mode,
                                                          int min_area) {
  const long P = B * HW;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < P; i += (long)gridDim.x * kBlock) {
    const long b = i / HW;
    const int v = lab[i];
    const int r = root[i];
    int o = v;
    if (r >= 0) {
      const long gr = b * HW + r;
      if (mode == 0) {
        // r >= 1 here: a component without a frame pixel does not contain pixel 0
        if (v == 0 && aux[gr] == 0 && r >= 1) o = lab[gr - 1];
      } else if (v != 0) {
        if (area[gr] < min_area) o = 0;
        if (key && (int)~(unsigned)(key[b * kCcKeyCols + v] & 0xffffffffull) != r) o = 0;
      }
    }
    out[i] = (uint8_t)o;
  }
}

// ---- lesion counters -------------------------------------------------------------------------------------------
// lab / root / area / aux [2N][HW]: planes [0, N) the prediction, [N, 2N) the target; aux = pixels of the component
// where the other source holds the same class.  grid (blocks per plane, 2N): an LDS histogram per class of
// (components, hits), then one integer atomic per non-empty bin into state [4][K] (rows: GT components, GT hits,
// predicted components, predicted hits) and, when given, per [N][K][4].
__global__ __launch_bounds__(kBlock) void cc_lesion_kernel(const uint8_t* __restrict__ lab,
                                                           const int* __restrict__ root, const int* __restrict__ area,
                                                           const int* __restrict__ aux, const int* __restrict__ err,
                                                           int64_t* __restrict__ state, int64_t* __restrict__ state_err,
                                                           int64_t* __restrict__ per, int N, int K, long HW,
                                                           double min_overlap) {
  __shared__ int s_hist[2 * kCcKeyCols];
  for (int k = threadIdx.x; k < 2 * K; k += kBlock) s_hist[k] = 0;
  __syncthreads();
  const long plane = blockIdx.y;
  const long base = plane * HW;
  for (long p = (long)blockIdx.x * kBlock + threadIdx.x; p < HW; p += (long)gridDim.x * kBlock) {
    const int v = lab[base + p];
    if (v < 1 || v > K || root[base + p] != (int)p) continue;
    const int a = area[base + p], it = aux[base + p];
    atomicAdd(&s_hist[2 * (v - 1)], 1);
    if (it >= 1 && (double)it >= min_overlap * (double)a) atomicAdd(&s_hist[2 * (v - 1) + 1], 1);
  }
  __syncthreads();
  const int row = plane < N ? 2 : 0;                       // predicted : ground truth
  const long n = plane < N ? plane : plane - N;
  for (int k = threadIdx.x; k < 2 * K; k += kBlock) {
    const int c = s_hist[k];
    if (c == 0) continue;
    const int cls = k >> 1, hit = k & 1;
    atomicAdd((unsigned long long*)(state + (long)(row + hit) * K + cls), (unsigned long long)c);
    if (per) atomicAdd((unsigned long long*)(per + (n * K + cls) * 4 + row + hit), (unsigned long long)c);
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && *err != 0)
    atomicAdd((unsigned long long*)state_err, (unsigned long long)*err);
}

// In-stream zero fill of the few words that atomics accumulate into (a kernel, not a memset node: the project keeps
// memsets out of anything a hipGraph may capture, see conv.hip).
__global__ __launch_bounds__(kBlock) void cc_zero_kernel(int* __restrict__ p, long n) {
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long)gridDim.x * kBlock) p[i] = 0;
}

int grid1d(long n) {
  long b = (n + kBlock - 1) / kBlock;
  return (int)(b > 16384 ? 16384 : (b < 1 ? 1 : b));
}
}  // namespace

void cc_label(const uint8_t* lab, int32_t* root, int32_t* area, int32_t* aux, int32_t* err, long half, long B, int H,
              int W, int connectivity, int mode, hipStream_t s) {
  const int tilesX = (W + kTile - 1) / kTile, tilesY = (H + kTile - 1) / kTile;
  const int nSR = (H - 1) / kTile, nSC = (W - 1) / kTile;
  const long HW = (long)H * W;
  const int cap = (int)HW, conn8 = connectivity == 8;
  hipLaunchKernelGGL(cc_zero_kernel, dim3(1), dim3(kBlock), 0, s, err, 1L);
  hipLaunchKernelGGL(cc_tile_kernel, dim3((unsigned)(B * tilesX * tilesY)), dim3(kBlock), 0, s, lab, root, area, aux,
                     err, half, B, H, W, tilesX, tilesY, conn8, mode, cap);
  const long seam = B * ((long)nSR * W + (long)nSC * H);
  if (seam > 0) {
    hipLaunchKernelGGL(cc_seam_kernel, dim3(grid1d(seam)), dim3(kBlock), 0, s, lab, root, err, B, H, W, nSR, nSC,
                       conn8, cap);
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(grid1d(B * HW)), dim3(kBlock), 0, s, root, area, aux, err, B, HW, cap);
  }
}

void cc_rank(const int32_t* root, int32_t* rank, int64_t* num, long B, long HW, hipStream_t s) {
  hipLaunchKernelGGL(cc_rank_kernel, dim3((unsigned)B), dim3(kBlock), 0, s, root, rank, num, HW);
}

void cc_gather(const int32_t* root, const int32_t* src, int32_t* out, long B, long HW, hipStream_t s) {
  hipLaunchKernelGGL(cc_gather_kernel, dim3(grid1d(B * HW)), dim3(kBlock), 0, s, root, src, out, B, HW);
}

void cc_largest(const uint8_t* lab, const int32_t* root, const int32_t* area, int64_t* key, long B, long HW,
                hipStream_t s) {
  hipLaunchKernelGGL(cc_zero_kernel, dim3(grid1d(B * kCcKeyCols * 2)), dim3(kBlock), 0, s, (int*)key,
                     B * kCcKeyCols * 2);
  hipLaunchKernelGGL(cc_largest_kernel, dim3(grid1d(B * HW)), dim3(kBlock), 0, s, lab, root, area,
                     (unsigned long long*)key, B, HW);
}

void cc_apply(const uint8_t* lab, const int32_t* root, const int32_t* area, const int32_t* aux, const int64_t* key,
              uint8_t* out, long B, long HW, int mode, int min_area, hipStream_t s) {
  hipLaunchKernelGGL(cc_apply_kernel, dim3(grid1d(B * HW)), dim3(kBlock), 0, s, lab, root, area, aux,
                     (const unsigned long long*)key, out, B, HW, mode, min_area);
}

void cc_lesion(const uint8_t* lab, const int32_t* root, const int32_t* area, const int32_t* aux, const int32_t* err,
               int64_t* state, int64_t* state_err, int64_t* per, int N, int K, long HW, double min_overlap,
               hipStream_t s) {
  long bx = (HW + kBlock * 8 - 1) / (kBlock * 8);
  if (bx > 64) bx = 64;
  hipLaunchKernelGGL(cc_lesion_kernel, dim3((unsigned)bx, (unsigned)(2 * N)), dim3(kBlock), 0, s, lab, root, area, aux,
                     err, state, state_err, per, N, K, HW, min_overlap);
}
