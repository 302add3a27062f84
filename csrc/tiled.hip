// Sliding-window inference with flip test-time augmentation: everything around the network's forward.  An addition
// over the reference, which runs one whole-image forward.  Window index m = ((n * ny + iy) * nx + ix) * V + v; view v
// mirrors the WINDOW along x (fh) and / or y (fv), and entry (ky, kx) of its logits belongs to window pixel
// (fv ? wh - 1 - ky : ky, fh ? ww - 1 - kx : kx).  Image pixel (y, x) is pixel (y + py, x + px) of the zero-padded
// frame the window starts refer to (py = px = 0 unless the image is smaller than the window).
//   window_gather            images -> windows [m0, m0 + B): crop, zero padding and mirror in one copy
//   window_blend_accumulate  acc[n, c, y, x] += wy * wx * f(logit) over the windows of the chunk that cover the pixel,
//                            in ascending m; every pixel is owned by one thread, so no atomics and the fp32 sequence
//                            per pixel is the same however the windows were chunked (the stored partial sum is the
//                            register partial sum).  f = identity, or softmax over C / sigmoid in registers.
//   window_blend_finalize    acc / (V * ysum[y] * xsum[x]), and back to logits in probs mode
// Every index that reaches memory is checked against the tensor extents in the kernel, whatever the start and
// cover tables hold.
#include <float.h>

#include "common.h"
#include "launchers.h"

namespace {
constexpr int kBlock = 256;

struct TileGeo {
  int N, C, H, W, wh, ww, ny, nx, py, px, V, flips;
  long m0, B, M;   // this chunk holds windows [m0, m0 + B); M = N * ny * nx * V windows exist
};

DEVI void view_flips(int flips, int v, bool& fh, bool& fv) {
  fh = flips == 1 ? v != 0 : (flips == 3 ? (v & 1) != 0 : false);
  fv = flips == 2 ? v != 0 : (flips == 3 ? (v & 2) != 0 : false);
}

int grid1d(long n) {
  const long b = (n + kBlock - 1) / kBlock;
  return (int)(b > 32768 ? 32768 : (b < 1 ? 1 : b));
}

// One thread per VEC consecutive kx of one (window, channel, ky) row of the output.
template <int VEC>
__global__ __launch_bounds__(kBlock) void window_gather_kernel(const float* __restrict__ img, float* __restrict__ out,
                                                               const int* __restrict__ starts, TileGeo g) {
  const int gw = g.ww / VEC;                       // VEC == 4 only when ww % 4 == 0
  const long total = g.B * g.C * g.wh * gw;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long)gridDim.x * kBlock) {
    const int xg = (int)(i % gw);
    long r = i / gw;
    const int ky = (int)(r % g.wh);
    r /= g.wh;
    const int c = (int)(r % g.C);
    const long b = r / g.C, m = g.m0 + b;
    float val[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) val[j] = 0.f;
    if (m < g.M) {
      const int v = (int)(m % g.V);
      long q = m / g.V;
      const int ix = (int)(q % g.nx);
      q /= g.nx;
      const int iy = (int)(q % g.ny);
      const long n = q / g.ny;
      bool fh, fv;
      view_flips(g.flips, v, fh, fv);
      const int y = starts[iy] + (fv ? g.wh - 1 - ky : ky) - g.py;
      if (y >= 0 && y < g.H) {
        const float* row = img + ((n * g.C + c) * g.H + y) * (long)g.W;
        const int xb = starts[g.ny + ix] - g.px;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const int kx = xg * VEC + j;
          const int x = xb + (fh ? g.ww - 1 - kx : kx);
          if (x >= 0 && x < g.W) val[j] = row[x];
        }
      }
    }
    float* o = out + ((b * g.C + c) * g.wh + ky) * (long)g.ww + (long)xg * VEC;
    if (VEC == 4) {
      *reinterpret_cast<float4*>(o) = make_float4(val[0], val[1], val[2], val[3]);
    } else {
      o[0] = val[0];
    }
  }
}

DEVI float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// Coordinates of one work item: VEC consecutive pixels of image row (n, y) and the windows that can cover them.
struct Item {
  long n;
  int y, x0, iylo, iyhi, ixlo, ixhi;
  bool any;
};

template <int VEC>
DEVI Item decode_item(long i, const int* __restrict__ cover, const TileGeo& g, int n0, int y0, int rows) {
  Item t;
  const int gw = (g.W + VEC - 1) / VEC;
  t.x0 = (int)(i % gw) * VEC;
  const long r = i / gw;
  t.y = y0 + (int)(r % rows);
  t.n = n0 + r / rows;
  const int x1 = min(t.x0 + VEC - 1, g.W - 1);
  t.iylo = max(cover[t.y], 0);
  t.iyhi = min(cover[g.H + t.y], g.ny - 1);
  t.ixlo = max(cover[2 * g.H + t.x0], 0);
  t.ixhi = min(cover[2 * g.H + g.W + x1], g.nx - 1);
  // the first and the last window index that can touch these pixels against the chunk
  const long mlo = ((t.n * g.ny + t.iylo) * g.nx + t.ixlo) * g.V;
  const long mhi = ((t.n * g.ny + t.iyhi) * g.nx + t.ixhi) * g.V + g.V - 1;
  t.any = t.iylo <= t.iyhi && t.ixlo <= t.ixhi && mhi >= g.m0 && mlo < g.m0 + g.B;
  return t;
}

// C classes in registers (C = 1 .. 4), VEC pixels per thread; VEC == 4 needs W % 4 == 0 (16-byte accumulator rows).
template <int C, bool PROBS, int VEC>
__global__ __launch_bounds__(kBlock) void window_blend_kernel(const float* __restrict__ logits, float* __restrict__ acc,
                                                              const int* __restrict__ starts,
                                                              const int* __restrict__ cover,
                                                              const float* __restrict__ wy,
                                                              const float* __restrict__ wx, TileGeo g, int n0, int nimg,
                                                              int y0, int rows) {
  const int gw = (g.W + VEC - 1) / VEC;
  const long total = (long)nimg * rows * gw;
  const long plane = (long)g.H * g.W, wplane = (long)g.wh * g.ww;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long)gridDim.x * kBlock) {
    const Item t = decode_item<VEC>(i, cover, g, n0, y0, rows);
    if (!t.any) continue;
    float* a = acc + (t.n * C * g.H + t.y) * (long)g.W + t.x0;
    float s[C][VEC];
    if (VEC == 4) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float4 q = *reinterpret_cast<const float4*>(a + c * plane);
        s[c][0] = q.x; s[c][1] = q.y; s[c][2] = q.z; s[c][3] = q.w;
      }
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) s[c][0] = a[c * plane];
    }
    for (int iy = t.iylo; iy <= t.iyhi; ++iy) {
      const int ky = t.y + g.py - starts[iy];
      if ((unsigned)ky >= (unsigned)g.wh) continue;
      const float wyv = wy[ky];
      for (int ix = t.ixlo; ix <= t.ixhi; ++ix) {
        const int kx0 = t.x0 + g.px - starts[g.ny + ix];
        const long mb = ((t.n * g.ny + iy) * g.nx + ix) * g.V;
        for (int v = 0; v < g.V; ++v) {
          const long m = mb + v;
          if (m < g.m0 || m >= g.m0 + g.B) continue;
          bool fh, fv;
          view_flips(g.flips, v, fh, fv);
          const float* src = logits + ((m - g.m0) * C * g.wh + (fv ? g.wh - 1 - ky : ky)) * (long)g.ww;
#pragma unroll
          for (int j = 0; j < VEC; ++j) {
            const int kx = kx0 + j;
            if ((unsigned)kx >= (unsigned)g.ww || t.x0 + j >= g.W) continue;
            const float* p = src + (fh ? g.ww - 1 - kx : kx);
            const float w = wyv * wx[kx];
            float f[C];
#pragma unroll
            for (int c = 0; c < C; ++c) f[c] = p[c * wplane];
            if (PROBS) {
              if (C == 1) {
                f[0] = sigmoidf(f[0]);
              } else {
                float mx = f[0];
#pragma unroll
                for (int c = 1; c < C; ++c) mx = fmaxf(mx, f[c]);
                float sum = 0.f;
#pragma unroll
                for (int c = 0; c < C; ++c) { f[c] = expf(f[c] - mx); sum += f[c]; }
#pragma unroll
                for (int c = 0; c < C; ++c) f[c] = f[c] / sum;
              }
            }
#pragma unroll
            for (int c = 0; c < C; ++c) s[c][j] += w * f[c];
          }
        }
      }
    }
    if (VEC == 4) {
#pragma unroll
      for (int c = 0; c < C; ++c)
        *reinterpret_cast<float4*>(a + c * plane) = make_float4(s[c][0], s[c][1], s[c][2], s[c][3]);
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) a[c * plane] = s[c][0];
    }
  }
}

// Any C (<= kTileMaxClasses): one pixel per thread, nothing indexed by a loop variable kept in registers.  Logits
// mode sums one class at a time in a register; probs mode takes the window's maximum and exponential sum first and
// then adds class by class onto the stored sum -- the same fp32 sequence per (pixel, class) as the register form.
template <bool PROBS>
__global__ __launch_bounds__(kBlock) void window_blend_generic_kernel(const float* __restrict__ logits,
                                                                      float* __restrict__ acc,
                                                                      const int* __restrict__ starts,
                                                                      const int* __restrict__ cover,
                                                                      const float* __restrict__ wy,
                                                                      const float* __restrict__ wx, TileGeo g, int n0,
                                                                      int nimg, int y0, int rows) {
  const long total = (long)nimg * rows * g.W;
  const long plane = (long)g.H * g.W, wplane = (long)g.wh * g.ww;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long)gridDim.x * kBlock) {
    const Item t = decode_item<1>(i, cover, g, n0, y0, rows);
    if (!t.any) continue;
    float* a = acc + (t.n * g.C * g.H + t.y) * (long)g.W + t.x0;
    for (int pass = 0; pass < (PROBS ? 1 : g.C); ++pass) {
      float s = PROBS ? 0.f : a[pass * plane];
      for (int iy = t.iylo; iy <= t.iyhi; ++iy) {
        const int ky = t.y + g.py - starts[iy];
        if ((unsigned)ky >= (unsigned)g.wh) continue;
        const float wyv = wy[ky];
        for (int ix = t.ixlo; ix <= t.ixhi; ++ix) {
          const int kx = t.x0 + g.px - starts[g.ny + ix];
          if ((unsigned)kx >= (unsigned)g.ww) continue;
          const float w = wyv * wx[kx];
          const long mb = ((t.n * g.ny + iy) * g.nx + ix) * g.V;
          for (int v = 0; v < g.V; ++v) {
            const long m = mb + v;
            if (m < g.m0 || m >= g.m0 + g.B) continue;
            bool fh, fv;
            view_flips(g.flips, v, fh, fv);
            const float* p = logits + ((m - g.m0) * g.C * g.wh + (fv ? g.wh - 1 - ky : ky)) * (long)g.ww +
                             (fh ? g.ww - 1 - kx : kx);
            if (!PROBS) {
              s += w * p[pass * wplane];
            } else {
              float mx = p[0];
              for (int c = 1; c < g.C; ++c) mx = fmaxf(mx, p[c * wplane]);
              float sum = 0.f;
              for (int c = 0; c < g.C; ++c) sum += expf(p[c * wplane] - mx);
              for (int c = 0; c < g.C; ++c) a[c * plane] += w * (expf(p[c * wplane] - mx) / sum);
            }
          }
        }
      }
      if (!PROBS) a[pass * plane] = s;
    }
  }
}

DEVI float finalize1(float s, float den, int C, bool probs) {
  float p = s / den;
  if (probs) {
    if (C == 1) {
      p = fminf(fmaxf(p, FLT_MIN), 1.f - 0x1p-24f);
      p = logf(p / (1.f - p));
    } else {
      p = logf(fmaxf(p, FLT_MIN));
    }
  }
  return p;
}

template <int VEC>
__global__ __launch_bounds__(kBlock) void window_finalize_kernel(float* __restrict__ acc,
                                                                 const float* __restrict__ ysum,
                                                                 const float* __restrict__ xsum, long planes, int C,
                                                                 int H, int W, float views, bool probs) {
  const int gw = W / VEC;                          // VEC == 4 only when W % 4 == 0
  const long total = planes * H * gw;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long)gridDim.x * kBlock) {
    const int x0 = (int)(i % gw) * VEC;
    const long r = i / gw;                         // plane * H + y
    const int y = (int)(r % H);
    float* a = acc + r * W + x0;
    const float ys = ysum[y];
    if (VEC == 4) {
      float4 q = *reinterpret_cast<const float4*>(a);
      const float4 xs = *reinterpret_cast<const float4*>(xsum + x0);
      q.x = finalize1(q.x, ys * xs.x * views, C, probs);
      q.y = finalize1(q.y, ys * xs.y * views, C, probs);
      q.z = finalize1(q.z, ys * xs.z * views, C, probs);
      q.w = finalize1(q.w, ys * xs.w * views, C, probs);
      *reinterpret_cast<float4*>(a) = q;
    } else {
      a[0] = finalize1(a[0], ys * xsum[x0] * views, C, probs);
    }
  }
}

TileGeo make_geo(int N, int C, int H, int W, int wh, int ww, int ny, int nx, int py, int px, int flips, long m0,
                 long B) {
  TileGeo g;
  g.N = N; g.C = C; g.H = H; g.W = W; g.wh = wh; g.ww = ww; g.ny = ny; g.nx = nx; g.py = py; g.px = px;
  g.flips = flips;
  g.V = flips == 0 ? 1 : (flips == 3 ? 4 : 2);
  g.m0 = m0; g.B = B;
  g.M = (long)N * ny * nx * g.V;
  return g;
}

template <int C, bool PROBS>
void launch_blend(bool vec, long total1, long total4, hipStream_t s, const float* logits, float* acc, const int* starts,
                  const int* cover, const float* wy, const float* wx, const TileGeo& g, int n0, int nimg, int y0,
                  int rows) {
  if (vec)
    hipLaunchKernelGGL((window_blend_kernel<C, PROBS, 4>), dim3(grid1d(total4)), dim3(kBlock), 0, s, logits, acc,
                       starts, cover, wy, wx, g, n0, nimg, y0, rows);
  else
    hipLaunchKernelGGL((window_blend_kernel<C, PROBS, 1>), dim3(grid1d(total1)), dim3(kBlock), 0, s, logits, acc,
                       starts, cover, wy, wx, g, n0, nimg, y0, rows);
}
}  // namespace

void window_gather(const float* img, float* out, const int* starts, int N, int Cin, int H, int W, int wh, int ww,
                   int ny, int nx, int py, int px, int flips, long m0, long B, hipStream_t s) {
  const TileGeo g = make_geo(N, Cin, H, W, wh, ww, ny, nx, py, px, flips, m0, B);
  const bool vec = ww % 4 == 0 && ((uintptr_t)out & 15) == 0;
  const long total = B * Cin * wh * (vec ? ww / 4 : ww);
  if (vec)
    hipLaunchKernelGGL(window_gather_kernel<4>, dim3(grid1d(total)), dim3(kBlock), 0, s, img, out, starts, g);
  else
    hipLaunchKernelGGL(window_gather_kernel<1>, dim3(grid1d(total)), dim3(kBlock), 0, s, img, out, starts, g);
}

void window_blend_accumulate(const float* logits, float* acc, const int* starts, const int* cover, const float* wy,
                             const float* wx, int N, int C, int H, int W, int wh, int ww, int ny, int nx, int py,
                             int px, int flips, long m0, long B, bool probs, int n0, int n1, int y0, int y1,
                             hipStream_t s) {
  const TileGeo g = make_geo(N, C, H, W, wh, ww, ny, nx, py, px, flips, m0, B);
  const int nimg = n1 - n0, rows = y1 - y0;
  if (nimg <= 0 || rows <= 0) return;
  const bool vec = W % 4 == 0 && ((uintptr_t)acc & 15) == 0;
  const long total1 = (long)nimg * rows * W, total4 = (long)nimg * rows * ((W + 3) / 4);
#define BLEND_CASE(CC)                                                                                              \
  case CC:                                                                                                          \
    if (probs) launch_blend<CC, true>(vec, total1, total4, s, logits, acc, starts, cover, wy, wx, g, n0, nimg, y0,  \
                                      rows);                                                                        \
    else launch_blend<CC, false>(vec, total1, total4, s, logits, acc, starts, cover, wy, wx, g, n0, nimg, y0, rows); \
    break;
  switch (C) {
    BLEND_CASE(1)
    BLEND_CASE(2)
    BLEND_CASE(3)
    BLEND_CASE(4)
    default:
      if (probs)
        hipLaunchKernelGGL(window_blend_generic_kernel<true>, dim3(grid1d(total1)), dim3(kBlock), 0, s, logits, acc,
                           starts, cover, wy, wx, g, n0, nimg, y0, rows);
      else
        hipLaunchKernelGGL(window_blend_generic_kernel<false>, dim3(grid1d(total1)), dim3(kBlock), 0, s, logits, acc,
                           starts, cover, wy, wx, g, n0, nimg, y0, rows);
  }
#undef BLEND_CASE
}

void window_blend_finalize(float* acc, const float* ysum, const float* xsum, int N, int C, int H, int W, int V,
                           bool probs, hipStream_t s) {
  const long planes = (long)N * C;
  const bool vec = W % 4 == 0 && ((uintptr_t)acc & 15) == 0 && ((uintptr_t)xsum & 15) == 0;
  const long total = planes * H * (vec ? W / 4 : W);
  if (vec)
    hipLaunchKernelGGL(window_finalize_kernel<4>, dim3(grid1d(total)), dim3(kBlock), 0, s, acc, ysum, xsum, planes, C,
                       H, W, (float)V, probs);
  else
    hipLaunchKernelGGL(window_finalize_kernel<1>, dim3(grid1d(total)), dim3(kBlock), 0, s, acc, ysum, xsum, planes, C,
                       H, W, (float)V, probs);
}
