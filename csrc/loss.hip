// Fused losses over NCHW fp32 logits (one pass computes the loss partials AND the gradient).
//   ce_fwd_bwd    : nn.CrossEntropyLoss(weight, ignore_index) with mean reduction; also emits the
//                   per-pixel loss for OHEM (reference core/loss.py:6-31).
//   kd_kl_fwd_bwd : F.kl_div(log_softmax(s/T), softmax(t/T)) * T^2, elementwise-mean reduction
//                   (reference core/loss.py:42-46).
//   mse_fwd_bwd   : F.mse_loss(s, t) (KD 'mse', reference core/loss.py:47-48).
//   bce_dice_*    : binary (num_class == 1) BCE-with-logits + per-sample soft Dice on the sigmoid
//                   (SURVEY Appendix E.1): a per-sample reduction pass, then the gradient pass once the
//                   sample's Dice sums are known.
//   region_*      : softmax heads (num_class >= 2): CE | focal pixel term + per-sample, per-class soft
//                   Dice | Tversky on the softmax; statistics pass, one-block finalize (coefficients and
//                   loss stay on the device), gradient pass.
//   boundary_*    : softmax heads: the softmax integrated against the signed distance map of the labels
//                   (surface.hip sdf_sq); forward partials, one-block finalize, gradient pass.
// Partials are per block ([nblk][2] = {weighted loss sum, weight sum}); the host sums them.
#include "common.h"
#include "launchers.h"

namespace {
constexpr int kBlock = 256;
constexpr int kMaxC = 64;

__global__ __launch_bounds__(kBlock) void ce_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                    const float* __restrict__ weight, float* __restrict__ grad,
                                                    float* __restrict__ pix_loss, float* __restrict__ part, int N,
                                                    int C, long HW, int ignore_index) {
  __shared__ float red[2][kBlock / 64];
  const long P = (long)N * HW;
  float ls = 0.f, ws = 0.f;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < P; i += (long)gridDim.x * kBlock) {
    const long n = i / HW, p = i - n * HW;
    const float* x = logits + n * C * HW + p;
    float* gx = grad + n * C * HW + p;
    const long t = target[i];
    if (t == ignore_index || t < 0 || t >= C) {
      for (int c = 0; c < C; ++c) gx[c * HW] = 0.f;
      if (pix_loss) pix_loss[i] = 0.f;
      continue;
    }
    float m = -INFINITY;
    for (int c = 0; c < C; ++c) m = fmaxf(m, x[c * HW]);
    // full-precision exp/log (the per-pixel losses rank pixels for OHEM: fast-math ulps reorder
    // near-equal confident pixels against the torch oracle)
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += expf(x[c * HW] - m);
    const float lse = m + logf(se);
    const float l = lse - x[t * HW];
    const float w = weight ? weight[t] : 1.f;
    ls += w * l;
    ws += w;
    if (pix_loss) pix_loss[i] = l;
    const float inv = 1.f / se;
    for (int c = 0; c < C; ++c) {
      const float pc = expf(x[c * HW] - m) * inv;
      gx[c * HW] = w * (pc - (c == t ? 1.f : 0.f));
    }
  }
  ls = wave_sum(ls);
  ws = wave_sum(ws);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = ls; red[1][threadIdx.x >> 6] = ws; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f, b = 0.f;
    for (int w = 0; w < kBlock / 64; ++w) { a += red[0][w]; b += red[1][w]; }
    part[2 * blockIdx.x] = a;
    part[2 * blockIdx.x + 1] = b;
  }
}

__global__ __launch_bounds__(kBlock) void kd_kl_kernel(const float* __restrict__ s, const float* __restrict__ t,
                                                       float* __restrict__ grad, float* __restrict__ part, int N,
                                                       int C, long HW, float T) {
  __shared__ float red[kBlock / 64];
  const long P = (long)N * HW;
  const float invT = 1.f / T;
  const float gscale = T / (float)((double)N * C * HW);
  float acc = 0.f;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < P; i += (long)gridDim.x * kBlock) {
    const long n = i / HW, p = i - n * HW;
    const float* xs = s + n * C * HW + p;
    const float* xt = t + n * C * HW + p;
    float ms = -INFINITY, mt = -INFINITY;
    for (int c = 0; c < C; ++c) { ms = fmaxf(ms, xs[c * HW] * invT); mt = fmaxf(mt, xt[c * HW] * invT); }
    float ss = 0.f, st = 0.f;
    for (int c = 0; c < C; ++c) { ss += __expf(xs[c * HW] * invT - ms); st += __expf(xt[c * HW] * invT - mt); }
    const float lss = ms + __logf(ss), lst = mt + __logf(st);
    for (int c = 0; c < C; ++c) {
      const float lq = xs[c * HW] * invT - lss;   // log q (student)
      const float lp = xt[c * HW] * invT - lst;   // log p (teacher)
      const float pc = __expf(lp);
      acc += pc > 0.f ? pc * (lp - lq) : 0.f;
      grad[n * C * HW + c * HW + p] = gscale * (__expf(lq) - pc);
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f;
    for (int w = 0; w < kBlock / 64; ++w) a += red[w];
    part[blockIdx.x] = a;
  }
}
__global__ __launch_bounds__(kBlock) void mse_kernel(const float* __restrict__ s, const float* __restrict__ t,
                                                     float* __restrict__ grad, float* __restrict__ part, long n) {
  __shared__ float red[kBlock / 64];
  const float gs = 2.f / (float)n;
  float acc = 0.f;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long)gridDim.x * kBlock) {
    const float d = s[i] - t[i];
    acc += d * d;
    grad[i] = gs * d;
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f;
    for (int w = 0; w < kBlock / 64; ++w) a += red[w];
    part[blockIdx.x] = a;
  }
}

DEVI float sigmoidf(float x) { return 1.f / (1.f + __expf(-x)); }

// grid (splits, N): block (b, n) reduces its slice of sample n into part[n][b][4] =
// {sum BCE, sum p*t, sum p, sum t}.
__global__ __launch_bounds__(kBlock) void bce_dice_stats_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                                float* __restrict__ part, long HW) {
  __shared__ float red[4][kBlock / 64];
  const int n = blockIdx.y;
  const float* xs = x + (long)n * HW;
  const float* ts = t + (long)n * HW;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < HW; i += (long)gridDim.x * kBlock) {
    const float v = xs[i], y = ts[i];
    const float p = sigmoidf(v);
    a[0] += fmaxf(v, 0.f) - v * y + log1pf(__expf(-fabsf(v)));
    a[1] += p * y;
    a[2] += p;
    a[3] += y;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float w = wave_sum(a[k]);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = w;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    float v = 0.f;
    for (int w = 0; w < kBlock / 64; ++w) v += red[threadIdx.x][w];
    part[((long)n * gridDim.x + blockIdx.x) * 4 + threadIdx.x] = v;
  }
}

// d/dx of  bw * mean(BCE) + dw * (1 - mean_n (2 I_n + s) / (D_n + s)),  scaled by the upstream
// gradient *gup (a device scalar: no host sync).  coef[n] = {D_n + s, 2 I_n + s}.
__global__ __launch_bounds__(kBlock) void bce_dice_grad_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                               const float* __restrict__ coef,
                                                               const float* __restrict__ gup, float* __restrict__ grad,
                                                               int N, long HW, float bw, float dw) {
  const long total = (long)N * HW;
  const float g0 = gup[0];
  const float kb = bw / (float)total, kd = dw / (float)N;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long)gridDim.x * kBlock) {
    const int n = (int)(i / HW);
    const float den = coef[2 * n], num = coef[2 * n + 1];
    const float p = sigmoidf(x[i]), y = t[i];
    const float gd = -kd * p * (1.f - p) * (2.f * y * den - num) / (den * den);
    grad[i] = g0 * (kb * (p - y) + gd);
  }
}

// ---- OHEM selection on the device (reference core/loss.py:13-20): loss_hard = L[L > thr]; if fewer
// than n_min = #valid // 16 survive, loss_hard = topk(L, n_min).  Both branches are evaluated with no
// host synchronisation (graph-capturable): counts/sums above thr, and an exact radix select of the
// n_min-th largest per-pixel loss (non-negative floats order like their uint32 bits) in four 8-bit
// passes.  Ties at the k-th value take the fractional weight (n_min - #greater) / #equal each, which
// gives torch's loss value exactly (torch picks an arbitrary subset of the ties).
// State words (uint32 / fp32 bit-casts): see kOh* below.  Partials per block, reduced in fixed order.
constexpr int kOhPrefix = 0, kOhK = 1, kOhCntAbove = 2, kOhSumAbove = 3, kOhNMin = 4, kOhMode = 5, kOhSel = 6,
              kOhWGt = 7, kOhWEq = 8, kOhLoss = 9, kOhWords = 16;

__global__ __launch_bounds__(kBlock) void ohem_count_kernel(const float* __restrict__ L, const int64_t* __restrict__ tgt,
                                                            long P, float thr, int ignore_index, float* __restrict__ bpart) {
  __shared__ float red[3][kBlock / 64];
  float c = 0.f, sm = 0.f, nv = 0.f;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < P; i += (long)gridDim.x * kBlock) {
    const float l = L[i];
    if (l > thr) { c += 1.f; sm += l; }
    nv += tgt[i] != ignore_index ? 1.f : 0.f;
  }
  c = wave_sum(c); sm = wave_sum(sm); nv = wave_sum(nv);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = c; red[1][threadIdx.x >> 6] = sm; red[2][threadIdx.x >> 6] = nv; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f, b = 0.f, d = 0.f;
    for (int w = 0; w < kBlock / 64; ++w) { a += red[0][w]; b += red[1][w]; d += red[2][w]; }
    bpart[3 * blockIdx.x] = a; bpart[3 * blockIdx.x + 1] = b; bpart[3 * blockIdx.x + 2] = d;
  }
}

// one block: fixed-order reduction of the count partials, n_min, radix-select state, histogram reset
__global__ __launch_bounds__(kBlock) void ohem_init_kernel(const float* __restrict__ bpart, int nblk,
                                                           unsigned* __restrict__ st, unsigned* __restrict__ hist) {
  if (threadIdx.x == 0) {
    double c = 0.0, sm = 0.0, nv = 0.0;
    for (int b = 0; b < nblk; ++b) { c += bpart[3 * b]; sm += bpart[3 * b + 1]; nv += bpart[3 * b + 2]; }
    const unsigned n_min = (unsigned)((long long)nv / 16);
    st[kOhPrefix] = 0u;
    st[kOhK] = n_min;
    st[kOhCntAbove] = (unsigned)c;
    st[kOhSumAbove] = __float_as_uint((float)sm);
    st[kOhNMin] = n_min;
  }
  hist[threadIdx.x] = 0u;
}

__global__ __launch_bounds__(kBlock) void ohem_hist_kernel(const float* __restrict__ L, long P, int shift,
                                                           const unsigned* __restrict__ st, unsigned* __restrict__ hist) {
  __shared__ unsigned h[256];
  h[threadIdx.x] = 0u;
  __syncthreads();
  const unsigned prefix = st[kOhPrefix];
  const int hs = shift + 8;   // bits above this digit must equal the decided prefix
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < P; i += (long)gridDim.x * kBlock) {
    const unsigned u = __float_as_uint(L[i]);
    if (hs >= 32 || (u >> hs) == (prefix >> hs)) atomicAdd(&h[(u >> shift) & 255u], 1u);
  }
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

// one block: the digit of the k-th largest among the candidates; k becomes its rank inside that digit
__global__ __launch_bounds__(kBlock) void ohem_pick_kernel(int shift, unsigned* __restrict__ st, unsigned* __restrict__ hist) {
  __shared__ unsigned cnt[256];
  cnt[threadIdx.x] = hist[threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned k = st[kOhK];
    unsigned above = 0u, b = 0u;
    for (int d = 255; d >= 0; --d) {
      if (above + cnt[d] >= k) { b = (unsigned)d; break; }
      above += cnt[d];
    }
    st[kOhK] = k > above ? k - above : 0u;
    st[kOhPrefix] |= b << shift;
  }
  __syncthreads();
  hist[threadIdx.x] = 0u;   // ready for the next digit
}

__global__ __launch_bounds__(kBlock) void ohem_topk_kernel(const float* __restrict__ L, long P,
                                                           const unsigned* __restrict__ st, float* __restrict__ bpart) {
  __shared__ float red[3][kBlock / 64];
  const float vk = __uint_as_float(st[kOhPrefix]);
  float sgt = 0.f, cgt = 0.f, ceq = 0.f;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < P; i += (long)gridDim.x * kBlock) {
    const float l = L[i];
    if (l > vk) { sgt += l; cgt += 1.f; }
    else if (l == vk) ceq += 1.f;
  }
  sgt = wave_sum(sgt); cgt = wave_sum(cgt); ceq = wave_sum(ceq);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sgt; red[1][threadIdx.x >> 6] = cgt; red[2][threadIdx.x >> 6] = ceq; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f, b = 0.f, d = 0.f;
    for (int w = 0; w < kBlock / 64; ++w) { a += red[0][w]; b += red[1][w]; d += red[2][w]; }
    bpart[3 * blockIdx.x] = a; bpart[3 * blockIdx.x + 1] = b; bpart[3 * blockIdx.x + 2] = d;
  }
}

// one thread: pick the branch, write the loss and the per-pixel backward weights
__global__ void ohem_finish_kernel(const float* __restrict__ bpart, int nblk, float thr, unsigned* __restrict__ st,
                                   float* __restrict__ loss) {
  double sgt = 0.0, cgt = 0.0, ceq = 0.0;
  for (int b = 0; b < nblk; ++b) { sgt += bpart[3 * b]; cgt += bpart[3 * b + 1]; ceq += bpart[3 * b + 2]; }
  const unsigned n_min = st[kOhNMin], c_above = st[kOhCntAbove];
  const float vk = __uint_as_float(st[kOhPrefix]);
  float l, sel, wgt, weq;
  unsigned mode;
  if (c_above >= n_min) {   // threshold branch: mean of the losses above thr
    mode = 0u;
    sel = thr;
    wgt = c_above > 0 ? 1.f / (float)c_above : 0.f;
    weq = 0.f;
    l = c_above > 0 ? __uint_as_float(st[kOhSumAbove]) * wgt : 0.f;
  } else {                  // top-k branch: the n_min largest (ties at the k-th value shared)
    mode = 1u;
    sel = vk;
    const double take_eq = (double)n_min - cgt;
    l = (float)((sgt + take_eq * (double)vk) / (double)n_min);
    wgt = 1.f / (float)n_min;
    weq = ceq > 0.0 ? (float)(take_eq / ceq) * wgt : 0.f;
  }
  st[kOhMode] = mode;
  st[kOhSel] = __float_as_uint(sel);
  st[kOhWGt] = __float_as_uint(wgt);
  st[kOhWEq] = __float_as_uint(weq);
  loss[0] = l;
}

// backward: grad_logits[n][c][p] *= g * w(L[n][p]) in place
__global__ __launch_bounds__(kBlock) void ohem_bwd_kernel(float* __restrict__ grad, const float* __restrict__ L,
                                                          const unsigned* __restrict__ st, const float* __restrict__ gup,
                                                          int N, int C, long HW) {
  const float sel = __uint_as_float(st[kOhSel]), wgt = __uint_as_float(st[kOhWGt]) * gup[0];
  const float weq = __uint_as_float(st[kOhWEq]) * gup[0];
  const long P = (long)N * HW;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < P; i += (long)gridDim.x * kBlock) {
    const float l = L[i];
    const float w = l > sel ? wgt : (l == sel ? weq : 0.f);
    const long n = i / HW, p = i - n * HW;
    float* gx = grad + n * C * HW + p;
    for (int c = 0; c < C; ++c) gx[c * HW] *= w;
  }
}

// ---- multi-class region losses (num_class >= 2): pixel term (CE or focal) + per-sample soft
// Dice / Tversky on the softmax.  Two passes, grid (splits, N) each:
//   region_stats_*  : part[n][b][2 + 3C] = {sum w*l, sum w, then (I, P, T) per class} of block b's slice
//   region_finalize : one block sums the splits in a fixed order -> coef {num, den} per (n, c), the
//                     batch's sum(w) at coef[2NC], and the loss scalar
//   region_grad_*   : recomputes the softmax, reads coef and the upstream gradient from device memory
// A pixel is valid iff t != ignore_index and 0 <= t < C (the ce_kernel rule).  No float atomics:
// wave shuffle, then LDS, then one row per block, so every run adds in the same order.
constexpr int kRegionPixNone = 0, kRegionPixCE = 1, kRegionPixFocal = 2;
constexpr int kFinBlock = 1024;

struct RegionPix {   // the pixel term of one valid pixel
  float l;           // -(1 - p_t)^gamma log p_t
  float G;           // dl/dx_k = G * ([k == t] - p_k)
};

// q = 1 - p_t (as the normalised sum over the other classes), lpt = log p_t = x_t - lse.
// Focal needs gamma >= 1 (gamma == 0 is routed to CE by the caller).
DEVI RegionPix region_pixel(int pix, float gamma, float q, float pt, float lpt) {
  RegionPix r;
  if (pix == kRegionPixFocal) {
    // q^(gamma - 1): q == 0 gives exp2(-inf) = 0 for gamma > 1; gamma == 1 must not evaluate 0 * inf
    const float pw1 = gamma == 2.f ? q : (gamma == 1.f ? 1.f : __builtin_amdgcn_exp2f((gamma - 1.f) * __log2f(q)));
    const float f = pw1 * q;
    r.l = -f * lpt;
    r.G = gamma * pw1 * pt * lpt - f;
  } else {
    r.l = -lpt;
    r.G = -1.f;
  }
  return r;
}

DEVI bool region_valid(long t, int C, int ignore_index) { return t != ignore_index && t >= 0 && t < C; }

// one valid pixel, C classes in registers (every index static: no scratch)
template <int C>
DEVI void region_stats_px(const float (&x)[C], int t, float w, int pix, float gamma, float (&a)[2 + 3 * C]) {
  float m = x[0];
#pragma unroll
  for (int c = 1; c < C; ++c) m = fmaxf(m, x[c]);
  float e[C], se = 0.f, so = 0.f, xt = 0.f, et = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    e[c] = __expf(x[c] - m);
    se += e[c];
    if (c == t) { xt = x[c]; et = e[c]; } else so += e[c];
  }
  const float inv = 1.f / se;
  if (pix != kRegionPixNone) {
    const RegionPix r = region_pixel(pix, gamma, so * inv, et * inv, (xt - m) - __logf(se));
    a[0] += w * r.l;
    a[1] += w;
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float p = e[c] * inv;
    a[2 + 3 * c + 1] += p;
    if (c == t) { a[2 + 3 * c] += p; a[2 + 3 * c + 2] += 1.f; }
  }
}

template <int C, bool VEC>
__global__ __launch_bounds__(kBlock) void region_stats_kernel(const float* __restrict__ logits,
                                                              const int64_t* __restrict__ target,
                                                              const float* __restrict__ weight,
                                                              float* __restrict__ part, long HW, int ignore_index,
                                                              int pix, float gamma) {
  constexpr int F = 2 + 3 * C;
  __shared__ float red[F][kBlock / 64];
  const int n = blockIdx.y;
  const float* xs = logits + (long)n * C * HW;
  const int64_t* ts = target + (long)n * HW;
  float a[F];
#pragma unroll
  for (int k = 0; k < F; ++k) a[k] = 0.f;
  if (VEC) {   // 4 consecutive pixels of this sample per lane (HW % 4 == 0: a group never leaves the image)
    const long G = HW >> 2;
    for (long g = (long)blockIdx.x * kBlock + threadIdx.x; g < G; g += (long)gridDim.x * kBlock) {
      const longlong2 t01 = *reinterpret_cast<const longlong2*>(ts + 4 * g);
      const longlong2 t23 = *reinterpret_cast<const longlong2*>(ts + 4 * g + 2);
      const long tt[4] = {t01.x, t01.y, t23.x, t23.y};
      float4 xv[C];
#pragma unroll
      for (int c = 0; c < C; ++c) xv[c] = *reinterpret_cast<const float4*>(xs + c * HW + 4 * g);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!region_valid(tt[j], C, ignore_index)) continue;
        float x[C];
#pragma unroll
        for (int c = 0; c < C; ++c) x[c] = j == 0 ? xv[c].x : (j == 1 ? xv[c].y : (j == 2 ? xv[c].z : xv[c].w));
        region_stats_px<C>(x, (int)tt[j], weight ? weight[tt[j]] : 1.f, pix, gamma, a);
      }
    }
  } else {
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < HW; i += (long)gridDim.x * kBlock) {
      const long t = ts[i];
      if (!region_valid(t, C, ignore_index)) continue;
      float x[C];
#pragma unroll
      for (int c = 0; c < C; ++c) x[c] = xs[c * HW + i];
      region_stats_px<C>(x, (int)t, weight ? weight[t] : 1.f, pix, gamma, a);
    }
  }
#pragma unroll
  for (int k = 0; k < F; ++k) {
    const float w = wave_sum(a[k]);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = w;
  }
  __syncthreads();
  if (threadIdx.x < F) {
    float v = 0.f;
    for (int w = 0; w < kBlock / 64; ++w) v += red[threadIdx.x][w];
    part[((long)n * gridDim.x + blockIdx.x) * F + threadIdx.x] = v;
  }
}

// any C <= kMaxC, one pixel per lane: lane c of each wave keeps class c's (I, P, T) in registers and
// takes the wave's sum of every iteration (all lanes run every iteration; idle ones add zeros).
__global__ __launch_bounds__(kBlock) void region_stats_generic_kernel(const float* __restrict__ logits,
                                                                      const int64_t* __restrict__ target,
                                                                      const float* __restrict__ weight,
                                                                      float* __restrict__ part, int C, long HW,
                                                                      int ignore_index, int pix, float gamma) {
  __shared__ float red[kBlock / 64][kMaxC][3];
  __shared__ float red2[2][kBlock / 64];
  const int n = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int F = 2 + 3 * C;
  const float* xs = logits + (long)n * C * HW;
  const int64_t* ts = target + (long)n * HW;
  float aI = 0.f, aP = 0.f, aT = 0.f, ls = 0.f, ws = 0.f;
  for (long base = (long)blockIdx.x * kBlock; base < HW; base += (long)gridDim.x * kBlock) {
    const long i = base + threadIdx.x;
    const long t = i < HW ? ts[i] : -1;
    const bool valid = i < HW && region_valid(t, C, ignore_index);
    const float* xp = xs + (valid ? i : 0);
    float m = -INFINITY;
    for (int c = 0; c < C; ++c) m = fmaxf(m, xp[c * HW]);
    float se = 0.f, so = 0.f, xt = 0.f, et = 0.f;
    for (int c = 0; c < C; ++c) {
      const float v = xp[c * HW], e = __expf(v - m);
      se += e;
      if (c == t) { xt = v; et = e; } else so += e;
    }
    const float inv = 1.f / se;
    if (valid && pix != kRegionPixNone) {
      const float w = weight ? weight[t] : 1.f;
      const RegionPix r = region_pixel(pix, gamma, so * inv, et * inv, (xt - m) - __logf(se));
      ls += w * r.l;
      ws += w;
    }
    for (int c = 0; c < C; ++c) {
      const float p = valid ? __expf(xp[c * HW] - m) * inv : 0.f;
      const bool y = valid && c == t;
      const float sP = wave_sum(p), sI = wave_sum(y ? p : 0.f), sT = wave_sum(y ? 1.f : 0.f);
      if (lane == c) { aP += sP; aI += sI; aT += sT; }
    }
  }
  red[wv][lane][0] = aI; red[wv][lane][1] = aP; red[wv][lane][2] = aT;
  ls = wave_sum(ls);
  ws = wave_sum(ws);
  if (lane == 0) { red2[0][wv] = ls; red2[1][wv] = ws; }
  __syncthreads();
  float* row = part + ((long)n * gridDim.x + blockIdx.x) * F;
  if (threadIdx.x < 2) {
    float v = 0.f;
    for (int w = 0; w < kBlock / 64; ++w) v += red2[threadIdx.x][w];
    row[threadIdx.x] = v;
  }
  if (threadIdx.x < 3 * C) {
    const int c = threadIdx.x / 3, k = threadIdx.x - 3 * c;
    float v = 0.f;
    for (int w = 0; w < kBlock / 64; ++w) v += red[w][c][k];
    row[2 + threadIdx.x] = v;
  }
}

DEVI float block_sum_fin(float v, float* red) {   // kFinBlock threads, fixed order; every thread gets the total
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
  for (int w = 0; w < kFinBlock / 64; ++w) s += red[w];
  return s;
}

// one block: TI_nc = num / den with num = I + s, den = I + a (P - I) + b (T - I) + s;
// loss = pw * sum(w l) / sum(w) [0 when no pixel is valid] + rw * (1 - mean_{n, c >= c0} TI_nc)
__global__ __launch_bounds__(kFinBlock) void region_finalize_kernel(const float* __restrict__ part,
                                                                     float* __restrict__ coef,
                                                                     float* __restrict__ loss, int N, int C,
                                                                     int splits, float pw, float rw, float a, float b,
                                                                     float s, int c0) {
  __shared__ float red[kFinBlock / 64];
  const int F = 2 + 3 * C;
  float ti = 0.f;
  for (int idx = threadIdx.x; idx < N * C; idx += kFinBlock) {
    const int n = idx / C, c = idx - n * C;
    const float* p = part + (long)n * splits * F + 2 + 3 * c;
    float I = 0.f, P = 0.f, T = 0.f;
    for (int k = 0; k < splits; ++k) { I += p[(long)k * F]; P += p[(long)k * F + 1]; T += p[(long)k * F + 2]; }
    const float num = I + s, den = I + a * (P - I) + b * (T - I) + s;
    coef[2 * idx] = num;
    coef[2 * idx + 1] = den;
    if (c >= c0) ti += num / den;
  }
  float S = 0.f, W = 0.f;
  for (int n = threadIdx.x; n < N; n += kFinBlock) {
    const float* p = part + (long)n * splits * F;
    for (int k = 0; k < splits; ++k) { S += p[(long)k * F]; W += p[(long)k * F + 1]; }
  }
  ti = block_sum_fin(ti, red);
  S = block_sum_fin(S, red);
  W = block_sum_fin(W, red);
  if (threadIdx.x == 0) {
    coef[2 * N * C] = W;
    float l = 0.f;
    if (pw != 0.f && W > 0.f) l += pw * (S / W);
    if (rw != 0.f) l += rw * (1.f - ti / (float)(N * (C - c0)));
    loss[0] = l;
  }
}

// dTI/dp_c of one (n, c): k1 where y_c = 1, k0 where y_c = 0, both scaled by -rw / (N C')
DEVI void region_k(const float* coef, int n, int C, int c, int N, float rw, float a, float b, int c0, float& k1,
                   float& k0) {
  k1 = k0 = 0.f;
  if (rw == 0.f || c < c0) return;
  const float num = coef[2 * (n * C + c)], den = coef[2 * (n * C + c) + 1];
  const float sc = -rw / ((float)(N * (C - c0)) * den * den);
  k1 = sc * (den - num * (1.f - b));
  k0 = -sc * num * a;
}

// dx_k = g0 * (p_k (A_k - sum_c A_c p_c) + kp * G * ([k == t] - p_k)),  A_c = y_c ? k1_c : k0_c
template <int C>
DEVI void region_grad_px(const float (&x)[C], int t, float kp, int pix, float gamma, const float (&k1)[C],
                         const float (&k0)[C], float g0, float (&g)[C]) {
  float m = x[0];
#pragma unroll
  for (int c = 1; c < C; ++c) m = fmaxf(m, x[c]);
  float e[C], se = 0.f, so = 0.f, xt = 0.f, et = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    e[c] = __expf(x[c] - m);
    se += e[c];
    if (c == t) { xt = x[c]; et = e[c]; } else so += e[c];
  }
  const float inv = 1.f / se;
  float kG = 0.f;
  if (pix != kRegionPixNone) kG = kp * region_pixel(pix, gamma, so * inv, et * inv, (xt - m) - __logf(se)).G;
  float dot = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) dot += (c == t ? k1[c] : k0[c]) * (e[c] * inv);
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float p = e[c] * inv;
    g[c] = g0 * (p * ((c == t ? k1[c] : k0[c]) - dot) + kG * ((c == t ? 1.f : 0.f) - p));
  }
}

template <int C, bool VEC>
__global__ __launch_bounds__(kBlock) void region_grad_kernel(const float* __restrict__ logits,
                                                             const int64_t* __restrict__ target,
                                                             const float* __restrict__ weight,
                                                             const float* __restrict__ coef,
                                                             const float* __restrict__ gup, float* __restrict__ grad,
                                                             int N, long HW, int ignore_index, int pix, float gamma,
                                                             float pw, float rw, float a, float b, int c0) {
  const int n = blockIdx.y;
  const float* xs = logits + (long)n * C * HW;
  const int64_t* ts = target + (long)n * HW;
  float* gs = grad + (long)n * C * HW;
  const float g0 = gup[0], W = coef[2 * N * C];
  const float kpw = (pix != kRegionPixNone && W > 0.f) ? pw / W : 0.f;
  float k1[C], k0[C];
#pragma unroll
  for (int c = 0; c < C; ++c) region_k(coef, n, C, c, N, rw, a, b, c0, k1[c], k0[c]);
  if (VEC) {
    const long G = HW >> 2;
    for (long g = (long)blockIdx.x * kBlock + threadIdx.x; g < G; g += (long)gridDim.x * kBlock) {
      const longlong2 t01 = *reinterpret_cast<const longlong2*>(ts + 4 * g);
      const longlong2 t23 = *reinterpret_cast<const longlong2*>(ts + 4 * g + 2);
      const long tt[4] = {t01.x, t01.y, t23.x, t23.y};
      float4 xv[C];
#pragma unroll
      for (int c = 0; c < C; ++c) xv[c] = *reinterpret_cast<const float4*>(xs + c * HW + 4 * g);
      float o[C][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float x[C], gg[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
          x[c] = j == 0 ? xv[c].x : (j == 1 ? xv[c].y : (j == 2 ? xv[c].z : xv[c].w));
          gg[c] = 0.f;
        }
        if (region_valid(tt[j], C, ignore_index))
          region_grad_px<C>(x, (int)tt[j], kpw * (weight ? weight[tt[j]] : 1.f), pix, gamma, k1, k0, g0, gg);
#pragma unroll
        for (int c = 0; c < C; ++c) o[c][j] = gg[c];
      }
#pragma unroll
      for (int c = 0; c < C; ++c)
        *reinterpret_cast<float4*>(gs + c * HW + 4 * g) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
    }
  } else {
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < HW; i += (long)gridDim.x * kBlock) {
      const long t = ts[i];
      float x[C], gg[C];
#pragma unroll
      for (int c = 0; c < C; ++c) { x[c] = xs[c * HW + i]; gg[c] = 0.f; }
      if (region_valid(t, C, ignore_index))
        region_grad_px<C>(x, (int)t, kpw * (weight ? weight[t] : 1.f), pix, gamma, k1, k0, g0, gg);
#pragma unroll
      for (int c = 0; c < C; ++c) gs[c * HW + i] = gg[c];
    }
  }
}

__global__ __launch_bounds__(kBlock) void region_grad_generic_kernel(
    const float* __restrict__ logits, const int64_t* __restrict__ target, const float* __restrict__ weight,
    const float* __restrict__ coef, const float* __restrict__ gup, float* __restrict__ grad, int N, int C, long HW,
    int ignore_index, int pix, float gamma, float pw, float rw, float a, float b, int c0) {
  __shared__ float kk[kMaxC][2];
  const int n = blockIdx.y;
  const float* xs = logits + (long)n * C * HW;
  const int64_t* ts = target + (long)n * HW;
  float* gs = grad + (long)n * C * HW;
  if (threadIdx.x < C) region_k(coef, n, C, threadIdx.x, N, rw, a, b, c0, kk[threadIdx.x][0], kk[threadIdx.x][1]);
  __syncthreads();
  const float g0 = gup[0], W = coef[2 * N * C];
  const float kpw = (pix != kRegionPixNone && W > 0.f) ? pw / W : 0.f;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < HW; i += (long)gridDim.x * kBlock) {
    const long t = ts[i];
    const float* xp = xs + i;
    float* gp = gs + i;
    if (!region_valid(t, C, ignore_index)) {
      for (int c = 0; c < C; ++c) gp[c * HW] = 0.f;
      continue;
    }
    float m = -INFINITY;
    for (int c = 0; c < C; ++c) m = fmaxf(m, xp[c * HW]);
    float se = 0.f, so = 0.f, xt = 0.f, et = 0.f, dot = 0.f;
    for (int c = 0; c < C; ++c) {
      const float v = xp[c * HW], e = __expf(v - m);
      se += e;
      dot += kk[c][c == t ? 0 : 1] * e;
      if (c == t) { xt = v; et = e; } else so += e;
    }
    const float inv = 1.f / se;
    dot *= inv;
    float kG = 0.f;
    if (pix != kRegionPixNone)
      kG = kpw * (weight ? weight[t] : 1.f) * region_pixel(pix, gamma, so * inv, et * inv, (xt - m) - __logf(se)).G;
    for (int c = 0; c < C; ++c) {
      const float p = __expf(xp[c * HW] - m) * inv;
      gp[c * HW] = g0 * (p * (kk[c][c == t ? 0 : 1] - dot) + kG * ((c == t ? 1.f : 0.f) - p));
    }
  }
}

bool region_vec_ok(const void* x, const void* t, const void* g, long HW) {
  return HW % 4 == 0 && (((uintptr_t)x | (uintptr_t)t | (uintptr_t)g) & 15) == 0;
}

// ---- boundary (signed-distance) term: L = sum_{valid x, k < K} p_{c_k}(x) phi_k(x) / (K max(V, 1)), phi from the
// signed squared distance s [N][K][HW] (surface.hip sdf_sq): sqrt(s), 1 - sqrt(-s), 0.  The integer is exact in
// fp32 and the root correctly rounded, so phi is the same number wherever it is evaluated.  (sqrtf, not
// __fsqrt_rn: the HIP headers map the latter to the native, approximate root.)
//   boundary_fwd_*    : softmax in registers (C = 2, 3, 4) or re-read (generic), part[b] = {sum p phi, #valid}
//   boundary_finalize : one block adds the partials in a fixed order (fp64) -> loss and norm = 1 / (K max(V, 1))
//   boundary_grad_*   : dx_k = gup norm p_k (phi~_k - sum_c p_c phi~_c), phi~ = 0 for unlisted classes; 0 if invalid
DEVI float sdf_phi_of(int v) { return v > 0 ? sqrtf((float)v) : (v < 0 ? 1.f - sqrtf((float)-v) : 0.f); }

DEVI void boundary_block_out(float acc, float cnt, float* part) {
  __shared__ float red[2][kBlock / 64];
  acc = wave_sum(acc);
  cnt = wave_sum(cnt);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = acc; red[1][threadIdx.x >> 6] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f, b = 0.f;
    for (int w = 0; w < kBlock / 64; ++w) { a += red[0][w]; b += red[1][w]; }
    part[2 * blockIdx.x] = a;
    part[2 * blockIdx.x + 1] = b;
  }
}

template <int C>
__global__ __launch_bounds__(kBlock) void boundary_fwd_kernel(const float* __restrict__ logits,
                                                              const int64_t* __restrict__ target,
                                                              const int* __restrict__ sdf, SdfClasses cls, int K,
                                                              float* __restrict__ part, long P, long HW,
                                                              int ignore_index) {
  float acc = 0.f, cnt = 0.f;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < P; i += (long)gridDim.x * kBlock) {
    if (!region_valid(target[i], C, ignore_index)) continue;
    const long n = i / HW, p = i - n * HW;
    const float* xs = logits + n * C * HW + p;
    const int* sp = sdf + n * K * HW + p;
    float x[C];
#pragma unroll
    for (int c = 0; c < C; ++c) x[c] = xs[c * HW];
    float m = x[0];
#pragma unroll
    for (int c = 1; c < C; ++c) m = fmaxf(m, x[c]);
    float se = 0.f, dot = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float e = __expf(x[c] - m);
      se += e;
      const int k = cls.plane[c];
      if (k >= 0) dot += e * sdf_phi_of(sp[k * HW]);
    }
    acc += dot / se;
    cnt += 1.f;
  }
  boundary_block_out(acc, cnt, part);
}

__global__ __launch_bounds__(kBlock) void boundary_fwd_generic_kernel(const float* __restrict__ logits,
                                                                      const int64_t* __restrict__ target,
                                                                      const int* __restrict__ sdf, SdfClasses cls,
                                                                      int K, float* __restrict__ part, long P, int C,
                                                                      long HW, int ignore_index) {
  float acc = 0.f, cnt = 0.f;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < P; i += (long)gridDim.x * kBlock) {
    if (!region_valid(target[i], C, ignore_index)) continue;
    const long n = i / HW, p = i - n * HW;
    const float* xs = logits + n * C * HW + p;
    const int* sp = sdf + n * K * HW + p;
    float m = -INFINITY;
    for (int c = 0; c < C; ++c) m = fmaxf(m, xs[c * HW]);
    float se = 0.f, dot = 0.f;
    for (int c = 0; c < C; ++c) se += __expf(xs[c * HW] - m);
    for (int k = 0; k < K; ++k) dot += __expf(xs[cls.c[k] * HW] - m) * sdf_phi_of(sp[k * HW]);
    acc += dot / se;
    cnt += 1.f;
  }
  boundary_block_out(acc, cnt, part);
}

__global__ __launch_bounds__(kFinBlock) void boundary_finalize_kernel(const float* __restrict__ part, int nblk, int K,
                                                                       float* __restrict__ loss,
                                                                       float* __restrict__ norm) {
  __shared__ double red[2][kFinBlock];
  double s = 0.0, v = 0.0;
  for (int b = threadIdx.x; b < nblk; b += kFinBlock) { s += part[2 * b]; v += part[2 * b + 1]; }
  red[0][threadIdx.x] = s;
  red[1][threadIdx.x] = v;
  __syncthreads();
  for (int h = kFinBlock / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
      red[0][threadIdx.x] += red[0][threadIdx.x + h];
      red[1][threadIdx.x] += red[1][threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double V = red[1][0] > 1.0 ? red[1][0] : 1.0;
    const double k = 1.0 / ((double)K * V);
    loss[0] = (float)(red[0][0] * k);
    norm[0] = (float)k;
  }
}

template <int C>
__global__ __launch_bounds__(kBlock) void boundary_grad_kernel(const float* __restrict__ logits,
                                                               const int64_t* __restrict__ target,
                                                               const int* __restrict__ sdf, SdfClasses cls, int K,
                                                               const float* __restrict__ norm,
                                                               const float* __restrict__ gup, float* __restrict__ grad,
                                                               long P, long HW, int ignore_index) {
  const float g0 = gup[0] * norm[0];
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < P; i += (long)gridDim.x * kBlock) {
    const long n = i / HW, p = i - n * HW;
    float* gs = grad + n * C * HW + p;
    if (!region_valid(target[i], C, ignore_index)) {
#pragma unroll
      for (int c = 0; c < C; ++c) gs[c * HW] = 0.f;
      continue;
    }
    const float* xs = logits + n * C * HW + p;
    const int* sp = sdf + n * K * HW + p;
    float x[C], e[C], ph[C];
#pragma unroll
    for (int c = 0; c < C; ++c) x[c] = xs[c * HW];
    float m = x[0];
#pragma unroll
    for (int c = 1; c < C; ++c) m = fmaxf(m, x[c]);
    float se = 0.f, dot = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      e[c] = __expf(x[c] - m);
      se += e[c];
      const int k = cls.plane[c];
      ph[c] = k >= 0 ? sdf_phi_of(sp[k * HW]) : 0.f;
      dot += e[c] * ph[c];
    }
    const float inv = 1.f / se;
    dot *= inv;
#pragma unroll
    for (int c = 0; c < C; ++c) gs[c * HW] = g0 * (e[c] * inv) * (ph[c] - dot);
  }
}

__global__ __launch_bounds__(kBlock) void boundary_grad_generic_kernel(
    const float* __restrict__ logits, const int64_t* __restrict__ target, const int* __restrict__ sdf, SdfClasses cls,
    int K, const float* __restrict__ norm, const float* __restrict__ gup, float* __restrict__ grad, long P, int C,
    long HW, int ignore_index) {
  const float g0 = gup[0] * norm[0];
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < P; i += (long)gridDim.x * kBlock) {
    const long n = i / HW, p = i - n * HW;
    float* gs = grad + n * C * HW + p;
    if (!region_valid(target[i], C, ignore_index)) {
      for (int c = 0; c < C; ++c) gs[c * HW] = 0.f;
      continue;
    }
    const float* xs = logits + n * C * HW + p;
    const int* sp = sdf + n * K * HW + p;
    float m = -INFINITY;
    for (int c = 0; c < C; ++c) m = fmaxf(m, xs[c * HW]);
    float se = 0.f, dot = 0.f;
    for (int c = 0; c < C; ++c) se += __expf(xs[c * HW] - m);
    for (int k = 0; k < K; ++k) dot += __expf(xs[cls.c[k] * HW] - m) * sdf_phi_of(sp[k * HW]);
    const float inv = 1.f / se;
    dot *= inv;
    for (int c = 0; c < C; ++c) {
      const int k = cls.plane[c];
      const float ph = k >= 0 ? sdf_phi_of(sp[k * HW]) : 0.f;
      gs[c * HW] = g0 * (__expf(xs[c * HW] - m) * inv) * (ph - dot);
    }
  }
}
}  // namespace

long ce_blocks(long P) {
  long b = (P + kBlock * 8 - 1) / (kBlock * 8);
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  return b;
}

void ce_fwd_bwd(const float* logits, const int64_t* target, const float* weight, float* grad, float* pix_loss,
                float* part, int N, int C, long HW, int ignore_index, hipStream_t s) {
  (void)kMaxC;
  hipLaunchKernelGGL(ce_kernel, dim3(ce_blocks((long)N * HW)), dim3(kBlock), 0, s, logits, target, weight, grad,
                     pix_loss, part, N, C, HW, ignore_index);
}

void kd_kl_fwd_bwd(const float* s_logits, const float* t_logits, float* grad, float* part, int N, int C, long HW,
                   float T, hipStream_t s) {
  hipLaunchKernelGGL(kd_kl_kernel, dim3(ce_blocks((long)N * HW)), dim3(kBlock), 0, s, s_logits, t_logits, grad,
                     part, N, C, HW, T);
}

void mse_fwd_bwd(const float* s_, const float* t, float* grad, float* part, long n, hipStream_t s) {
  hipLaunchKernelGGL(mse_kernel, dim3(ce_blocks(n)), dim3(kBlock), 0, s, s_, t, grad, part, n);
}

int bce_dice_splits(long HW) {
  long b = (HW + kBlock * 16 - 1) / (kBlock * 16);
  if (b > 256) b = 256;
  if (b < 1) b = 1;
  return (int)b;
}

void bce_dice_stats(const float* x, const float* t, float* part, int N, long HW, hipStream_t s) {
  hipLaunchKernelGGL(bce_dice_stats_kernel, dim3(bce_dice_splits(HW), N), dim3(kBlock), 0, s, x, t, part, HW);
}

void bce_dice_grad(const float* x, const float* t, const float* coef, const float* gup, float* grad, int N, long HW,
                   float bw, float dw, hipStream_t s) {
  hipLaunchKernelGGL(bce_dice_grad_kernel, dim3(ce_blocks((long)N * HW)), dim3(kBlock), 0, s, x, t, coef, gup, grad,
                     N, HW, bw, dw);
}

int ohem_state_words() { return kOhWords; }

void ohem_select(const float* pix_loss, const int64_t* target, long P, float thr, int ignore_index, float* bpart,
                 unsigned* state, unsigned* hist, float* loss, hipStream_t s) {
  const int nblk = (int)ce_blocks(P);
  hipLaunchKernelGGL(ohem_count_kernel, dim3(nblk), dim3(kBlock), 0, s, pix_loss, target, P, thr, ignore_index, bpart);
  hipLaunchKernelGGL(ohem_init_kernel, dim3(1), dim3(kBlock), 0, s, bpart, nblk, state, hist);
  for (int shift = 24; shift >= 0; shift -= 8) {
    hipLaunchKernelGGL(ohem_hist_kernel, dim3(nblk), dim3(kBlock), 0, s, pix_loss, P, shift, state, hist);
    hipLaunchKernelGGL(ohem_pick_kernel, dim3(1), dim3(kBlock), 0, s, shift, state, hist);
  }
  hipLaunchKernelGGL(ohem_topk_kernel, dim3(nblk), dim3(kBlock), 0, s, pix_loss, P, state, bpart);
  hipLaunchKernelGGL(ohem_finish_kernel, dim3(1), dim3(1), 0, s, bpart, nblk, thr, state, loss);
}

void ohem_backward(float* grad, const float* pix_loss, const unsigned* state, const float* gup, int N, int C, long HW,
                   hipStream_t s) {
  hipLaunchKernelGGL(ohem_bwd_kernel, dim3(ce_blocks((long)N * HW)), dim3(kBlock), 0, s, grad, pix_loss, state, gup,
                     N, C, HW);
}

int boundary_blocks(long P) { return (int)ce_blocks(P); }

void boundary_fwd(const float* logits, const int64_t* target, const int32_t* sdf, const SdfClasses& cls, int K,
                  float* part, float* loss, float* norm, int N, int C, long HW, int ignore_index, hipStream_t s) {
  const long P = (long)N * HW;
  const int nblk = boundary_blocks(P);
  const dim3 grid(nblk), block(kBlock);
#define BOUNDARY_FWD(CC)                                                                                          \
  hipLaunchKernelGGL((boundary_fwd_kernel<CC>), grid, block, 0, s, logits, target, sdf, cls, K, part, P, HW,      \
                     ignore_index)
  if (C == 2) BOUNDARY_FWD(2);
  else if (C == 3) BOUNDARY_FWD(3);
  else if (C == 4) BOUNDARY_FWD(4);
  else
    hipLaunchKernelGGL(boundary_fwd_generic_kernel, grid, block, 0, s, logits, target, sdf, cls, K, part, P, C, HW,
                       ignore_index);
#undef BOUNDARY_FWD
  hipLaunchKernelGGL(boundary_finalize_kernel, dim3(1), dim3(kFinBlock), 0, s, part, nblk, K, loss, norm);
}

void boundary_grad(const float* logits, const int64_t* target, const int32_t* sdf, const SdfClasses& cls, int K,
                   const float* norm, const float* gup, float* grad, int N, int C, long HW, int ignore_index,
                   hipStream_t s) {
  const long P = (long)N * HW;
  const dim3 grid(boundary_blocks(P)), block(kBlock);
#define BOUNDARY_GRAD(CC)                                                                                         \
  hipLaunchKernelGGL((boundary_grad_kernel<CC>), grid, block, 0, s, logits, target, sdf, cls, K, norm, gup, grad, \
                     P, HW, ignore_index)
  if (C == 2) BOUNDARY_GRAD(2);
  else if (C == 3) BOUNDARY_GRAD(3);
  else if (C == 4) BOUNDARY_GRAD(4);
  else
    hipLaunchKernelGGL(boundary_grad_generic_kernel, grid, block, 0, s, logits, target, sdf, cls, K, norm, gup, grad,
                       P, C, HW, ignore_index);
#undef BOUNDARY_GRAD
}

int region_max_classes() { return kMaxC; }

int region_splits(long HW) {
  long b = (HW + kBlock * 16 - 1) / (kBlock * 16);
  if (b > 256) b = 256;
  if (b < 1) b = 1;
  return (int)b;
}

void region_stats(const float* logits, const int64_t* target, const float* weight, float* part, int N, int C,
                  long HW, int ignore_index, int pix, float gamma, hipStream_t s) {
  const dim3 grid(region_splits(HW), N), block(kBlock);
  const bool vec = region_vec_ok(logits, target, nullptr, HW);
#define REGION_STATS(CC)                                                                                          \
  if (vec)                                                                                                        \
    hipLaunchKernelGGL((region_stats_kernel<CC, true>), grid, block, 0, s, logits, target, weight, part, HW,      \
                       ignore_index, pix, gamma);                                                                 \
  else                                                                                                            \
    hipLaunchKernelGGL((region_stats_kernel<CC, false>), grid, block, 0, s, logits, target, weight, part, HW,     \
                       ignore_index, pix, gamma)
  if (C == 2) { REGION_STATS(2); }
  else if (C == 3) { REGION_STATS(3); }
  else if (C == 4) { REGION_STATS(4); }
  else
    hipLaunchKernelGGL(region_stats_generic_kernel, grid, block, 0, s, logits, target, weight, part, C, HW,
                       ignore_index, pix, gamma);
#undef REGION_STATS
}

void region_finalize(const float* part, float* coef, float* loss, int N, int C, int splits, float pw, float rw,
                     float a, float b, float smooth, int c0, hipStream_t s) {
  hipLaunchKernelGGL(region_finalize_kernel, dim3(1), dim3(kFinBlock), 0, s, part, coef, loss, N, C, splits, pw, rw,
                     a, b, smooth, c0);
}

void region_grad(const float* logits, const int64_t* target, const float* weight, const float* coef,
                 const float* gup, float* grad, int N, int C, long HW, int ignore_index, int pix, float gamma,
                 float pw, float rw, float a, float b, int c0, hipStream_t s) {
  const dim3 grid(region_splits(HW), N), block(kBlock);
  const bool vec = region_vec_ok(logits, target, grad, HW);
#define REGION_GRAD(CC)                                                                                           \
  if (vec)                                                                                                        \
    hipLaunchKernelGGL((region_grad_kernel<CC, true>), grid, block, 0, s, logits, target, weight, coef, gup,      \
                       grad, N, HW, ignore_index, pix, gamma, pw, rw, a, b, c0);                                  \
  else                                                                                                            \
    hipLaunchKernelGGL((region_grad_kernel<CC, false>), grid, block, 0, s, logits, target, weight, coef, gup,     \
                       grad, N, HW, ignore_index, pix, gamma, pw, rw, a, b, c0)
  if (C == 2) { REGION_GRAD(2); }
  else if (C == 3) { REGION_GRAD(3); }
  else if (C == 4) { REGION_GRAD(4); }
  else
    hipLaunchKernelGGL(region_grad_generic_kernel, grid, block, 0, s, logits, target, weight, coef, gup, grad, N, C,
                       HW, ignore_index, pix, gamma, pw, rw, a, b, c0);
#undef REGION_GRAD
}
