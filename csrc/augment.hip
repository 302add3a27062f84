// Train-time augmentation on the GPU over an HBM-resident uint8 dataset (reference
// datasets/polyp.py:37-47, albumentations semantics of SURVEY Appendix D as implemented on the host by
// utils/transforms.SegAugment -- the host draws every random number in the same order, the kernels
// only evaluate).  One batch =
//   aug_geometry   : RandomScale (image bilinear / mask nearest, the uint8 rounding of a resize) ->
//                    PadIfNeeded (centred BORDER_REFLECT_101) -> RandomCrop -> H/V flips, gathered
//                    per OUTPUT pixel straight from the variable-size source image (no intermediate
//                    scaled/padded copies);
//   aug_gray_mean  : per-sample mean of the gray image (ColorJitter contrast needs it at its position
//                    in the random op order; sliced fp64 partials + an in-order final sum);
//   aug_color      : one ColorJitter stage (brightness / contrast / saturation / hue per sample);
//   aug_finalize   : round (when jittered) + Normalize(mean, std) -> fp32 NCHW model input.
// Work buffer: fp32 [B][H*W][3] (RGB 0..255).  iparams (int32, kAugIParams per sample):
//   0 image index, 1 nh, 2 nw (scaled size), 3 pad top, 4 pad left, 5 crop y0, 6 crop x0, 7 hflip,
//   8 vflip, 9 jittered, 10..13 op code per stage (0 none, 1 brightness, 2 contrast, 3 saturation, 4 hue)
// fparams (fp32, 4 per sample): op value per stage.
// Opt-in additions (a batch in which some sample uses one; tables xi / xf described at the kernels below):
//   aug_warp       : aug_geometry with rotation / shift / cubic B-spline deformation composed into the gather;
//   aug_pointwise  : gamma and / or Philox Gaussian noise per pixel;
//   aug_blur       : separable Gaussian blur through an LDS tile, into a second work buffer.
#include "common.h"
#include "launchers.h"

namespace {
constexpr int kBlock = 256;

int grid_for(long n) {
  long b = (n + kBlock - 1) / kBlock;
  if (b > 16384) b = 16384;
  if (b < 1) b = 1;
  return (int)b;
}

DEVI int reflect101(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
  return i;
}

__global__ __launch_bounds__(kBlock) void aug_geometry_kernel(const uint8_t* __restrict__ images,
                                                              const uint8_t* __restrict__ masks,
                                                              const int64_t* __restrict__ meta,
                                                              const int* __restrict__ ip, float* __restrict__ work,
                                                              int64_t* __restrict__ mask_out, int B, int CH, int CW) {
  const long total = (long)B * CH * CW;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long)gridDim.x * kBlock) {
    const int b = (int)(i / ((long)CH * CW));
    const int pix = (int)(i - (long)b * CH * CW);
    const int oy = pix / CW, ox = pix - oy * CW;
    const int* q = ip + b * kAugIParams;
    const int img = q[0], nh = q[1], nw = q[2];
    const int64_t off = meta[4 * img], moff = meta[4 * img + 3];
    const int h = (int)meta[4 * img + 1], w = (int)meta[4 * img + 2];
    // flips act last in the reference pipeline: output (oy, ox) reads crop pixel (cy, cx)
    const int cy = q[8] ? CH - 1 - oy : oy;
    const int cx = q[7] ? CW - 1 - ox : ox;
    // crop -> padded canvas -> scaled image (reflect-101 padding)
    const int sy = reflect101(cy + q[5] - q[3], nh);
    const int sx = reflect101(cx + q[6] - q[4], nw);
    float rgb[3];
    uint8_t m;
    if (nh == h && nw == w) {
      const uint8_t* p = images + off + ((long)sy * w + sx) * 3;
      rgb[0] = p[0]; rgb[1] = p[1]; rgb[2] = p[2];
      m = masks[moff + (long)sy * w + sx];
    } else {
      // torch F.interpolate(bilinear, align_corners=False): src = max((dst + 0.5) * in/out - 0.5, 0)
      const float ry = (float)h / (float)nh, rx = (float)w / (float)nw;
      const float fy = fmaxf((sy + 0.5f) * ry - 0.5f, 0.f), fx = fmaxf((sx + 0.5f) * rx - 0.5f, 0.f);
      const int y0 = (int)fy, x0 = (int)fx;
      const int y1 = y0 + (y0 < h - 1), x1 = x0 + (x0 < w - 1);
      const float ly = fy - y0, lx = fx - x0;
      const uint8_t* r0 = images + off + (long)y0 * w * 3;
      const uint8_t* r1 = images + off + (long)y1 * w * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v = (1.f - ly) * ((1.f - lx) * r0[x0 * 3 + c] + lx * r0[x1 * 3 + c]) +
                        ly * ((1.f - lx) * r1[x0 * 3 + c] + lx * r1[x1 * 3 + c]);
        rgb[c] = fminf(fmaxf(rintf(v), 0.f), 255.f);        // resize of a uint8 image rounds
      }
      // nearest: src = min(floor(dst * in/out), in - 1)
      const int my = min((int)floorf(sy * ry), h - 1), mx = min((int)floorf(sx * rx), w - 1);
      m = masks[moff + (long)my * w + mx];
    }
    float* o = work + i * 3;
    o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2];
    mask_out[i] = m;
  }
}

DEVI float gray(const float* p) { return p[0] * 0.299f + p[1] * 0.587f + p[2] * 0.114f; }

// mean of each sample's gray image in fp64, deterministic: kGraySlices blocks per sample each reduce a
// fixed pixel slice (tree in LDS) to one fp64 partial, then one thread per sample adds its slices in
// order.  (One block per sample left 3/4 of the CUs idle: 155 us per launch at bs64 x 352^2.)
constexpr int kGraySlices = 16;

__global__ __launch_bounds__(kBlock) void aug_gray_partial_kernel(const float* __restrict__ work,
                                                                  double* __restrict__ part, int HW) {
  const int b = blockIdx.y, sl = blockIdx.x;
  const int per = (HW + kGraySlices - 1) / kGraySlices;
  const int i0 = sl * per, i1 = min(HW, i0 + per);
  const float* w = work + (long)b * HW * 3;
  double acc = 0.0;
  for (int i = i0 + threadIdx.x; i < i1; i += kBlock) acc += (double)gray(w + (long)i * 3);
  __shared__ double red[kBlock];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[(long)b * kGraySlices + sl] = red[0];
}

__global__ __launch_bounds__(kBlock) void aug_gray_final_kernel(const double* __restrict__ part,
                                                                float* __restrict__ mean, int B, int HW) {
  const int b = blockIdx.x * kBlock + threadIdx.x;
  if (b >= B) return;
  double t = 0.0;
  for (int sl = 0; sl < kGraySlices; ++sl) t += part[(long)b * kGraySlices + sl];
  mean[b] = (float)(t / HW);
}

DEVI float clip255(float v) { return fminf(fmaxf(v, 0.f), 255.f); }
DEVI float mod1(float x) { return x - floorf(x); }

DEVI void adjust_hue(float* px, float shift) {
  const float r = px[0] / 255.f, g = px[1] / 255.f, b = px[2] / 255.f;
  const float mx = fmaxf(r, fmaxf(g, b)), mn = fminf(r, fminf(g, b));
  const float d = mx - mn;
  float h = 0.f;
  if (d > 1e-12f) {
    const float rc = (mx - r) / d, gc = (mx - g) / d, bc = (mx - b) / d;
    h = r == mx ? bc - gc : (g == mx ? 2.f + rc - bc : 4.f + gc - rc);
    h = mod1(h / 6.f);
  }
  const float s = mx > 1e-12f ? d / mx : 0.f;
  const float v = mx;
  h = mod1(h + shift);
  const float fi = floorf(h * 6.f);
  const float f = h * 6.f - fi;
  const float p = v * (1.f - s), q = v * (1.f - s * f), t = v * (1.f - s * (1.f - f));
  int i = ((int)fi) % 6;
  if (i < 0) i += 6;
  float o0, o1, o2;
  switch (i) {
    case 0: o0 = v; o1 = t; o2 = p; break;
    case 1: o0 = q; o1 = v; o2 = p; break;
    case 2: o0 = p; o1 = v; o2 = t; break;
    case 3: o0 = p; o1 = q; o2 = v; break;
    case 4: o0 = t; o1 = p; o2 = v; break;
    default: o0 = v; o1 = p; o2 = q; break;
  }
  px[0] = clip255(o0 * 255.f); px[1] = clip255(o1 * 255.f); px[2] = clip255(o2 * 255.f);
}

__global__ __launch_bounds__(kBlock) void aug_color_kernel(float* __restrict__ work, const int* __restrict__ ip,
                                                           const float* __restrict__ fp, const float* __restrict__ mean,
                                                           int B, int HW, int stage) {
  const long total = (long)B * HW;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long)gridDim.x * kBlock) {
    const int b = (int)(i / HW);
    const int op = ip[b * kAugIParams + 10 + stage];
    if (op == 0) continue;
    const float v = fp[b * 4 + stage];
    float* px = work + i * 3;
    if (op == 1) {
#pragma unroll
      for (int c = 0; c < 3; ++c) px[c] = clip255(px[c] * v);
    } else if (op == 2) {
      const float m = mean[b];
#pragma unroll
      for (int c = 0; c < 3; ++c) px[c] = clip255((px[c] - m) * v + m);
    } else if (op == 3) {
      const float gr = gray(px);
#pragma unroll
      for (int c = 0; c < 3; ++c) px[c] = clip255((px[c] - gr) * v + gr);
    } else {
      adjust_hue(px, v);
    }
  }
}

__global__ __launch_bounds__(kBlock) void aug_finalize_kernel(const float* __restrict__ work,
                                                              const int* __restrict__ ip, float* __restrict__ out,
                                                              int B, int HW, float m0, float m1, float m2, float s0,
                                                              float s1, float s2) {
  const long total = (long)B * HW;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long)gridDim.x * kBlock) {
    const int b = (int)(i / HW);
    const long p = i - (long)b * HW;
    const bool rnd = ip[b * kAugIParams + 9] != 0;
    const float* px = work + i * 3;
    const float v0 = rnd ? rintf(px[0]) : px[0], v1 = rnd ? rintf(px[1]) : px[1], v2 = rnd ? rintf(px[2]) : px[2];
    float* o = out + (long)b * 3 * HW + p;
    o[0] = (v0 - m0) / s0;
    o[HW] = (v1 - m1) / s1;
    o[2 * (long)HW] = (v2 - m2) / s2;
  }
}

// ---- rotation / shift / B-spline warp, gamma, Gaussian blur, Gaussian noise (additions of this project;
// specification: utils/transforms.py warp_coords / warp_gather / medical_intensity).  Extra tables per sample:
//   xi (int32, kAugXI): 0 flags (kAugWarp | kAugElastic | kAugGamma | kAugBlur | kAugNoise | kAugConstant),
//                       1 B-spline cells n (1..8), 2 blur radius (1..8), 3 / 4 low / high word of the noise key
//   xf (fp32, kAugXF):  0..5 the 2x3 inverse-map matrix (rows y, x), 6 n / crop_h, 7 n / crop_w, 8 gamma,
//                       9 noise std, 10..18 blur taps w[0..8], 20.. the dy lattice (n+3)^2, 141.. the dx lattice
constexpr int kLattice = 121;            // (8 + 3)^2 control points per displacement component
constexpr int kXfLattice = 20;
constexpr float kCoordLimit = 32768.f;   // coordinates are clamped here before the float -> int conversion

DEVI int reflect101_any(int i, int n) {  // reflect101 for any distance from the image, without a loop
  if (n == 1) return 0;
  const int period = 2 * (n - 1);
  i %= period;
  if (i < 0) i += period;
  return i >= n ? period - i : i;
}

// One pixel (sy, sx) of the SCALED image, evaluated from the source exactly as aug_geometry_kernel does (the
// same expressions, so a sample that does not warp comes out bit for bit as on that path).
struct AugSrc {
  const uint8_t* img;
  const uint8_t* msk;
  int h, w, nh, nw;
};

DEVI void src_pixel(const AugSrc& s, int sy, int sx, float* rgb) {
  const int h = s.h, w = s.w;
  if (s.nh == h && s.nw == w) {
    const uint8_t* p = s.img + ((long)sy * w + sx) * 3;
    rgb[0] = p[0]; rgb[1] = p[1]; rgb[2] = p[2];
    return;
  }
  const float ry = (float)h / (float)s.nh, rx = (float)w / (float)s.nw;
  const float fy = fmaxf((sy + 0.5f) * ry - 0.5f, 0.f), fx = fmaxf((sx + 0.5f) * rx - 0.5f, 0.f);
  const int y0 = (int)fy, x0 = (int)fx;
  const int y1 = y0 + (y0 < h - 1), x1 = x0 + (x0 < w - 1);
  const float ly = fy - y0, lx = fx - x0;
  const uint8_t* r0 = s.img + (long)y0 * w * 3;
  const uint8_t* r1 = s.img + (long)y1 * w * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = (1.f - ly) * ((1.f - lx) * r0[x0 * 3 + c] + lx * r0[x1 * 3 + c]) +
                    ly * ((1.f - lx) * r1[x0 * 3 + c] + lx * r1[x1 * 3 + c]);
    rgb[c] = fminf(fmaxf(rintf(v), 0.f), 255.f);
  }
}

DEVI uint8_t src_mask(const AugSrc& s, int sy, int sx) {
  const int h = s.h, w = s.w;
  if (s.nh == h && s.nw == w) return s.msk[(long)sy * w + sx];
  const float ry = (float)h / (float)s.nh, rx = (float)w / (float)s.nw;
  const int my = min((int)floorf(sy * ry), h - 1), mx = min((int)floorf(sx * rx), w - 1);
  return s.msk[(long)my * w + mx];
}

// neighbour (y, x) of a warped sample through the border rule: reflect-101, or zeros outside the scaled image
DEVI void border_pixel(const AugSrc& s, int y, int x, bool constant, float* rgb) {
  if (constant) {
    if (y < 0 || y >= s.nh || x < 0 || x >= s.nw) {
      rgb[0] = rgb[1] = rgb[2] = 0.f;
      return;
    }
    src_pixel(s, y, x, rgb);
  } else {
    src_pixel(s, reflect101_any(y, s.nh), reflect101_any(x, s.nw), rgb);
  }
}

struct Basis { float b0, b1, b2, b3; };

// uniform cubic B-spline basis at u in [0, 1): the fp32 operation order of transforms._bspline_basis
DEVI Basis bspline_basis(float u) {
#pragma clang fp contract(off)
  const float sixth = 1.0f / 6.0f;
  const float t = 1.f - u, u2 = u * u, u3 = u2 * u;
  Basis b;
  b.b0 = ((t * t) * t) * sixth;
  b.b1 = ((3.f * u3 - 6.f * u2) + 4.f) * sixth;
  b.b2 = ((((-3.f * u3) + 3.f * u2) + 3.f * u) + 1.f) * sixth;
  b.b3 = u3 * sixth;
  return b;
}

DEVI float bspline_row(const float* p, const Basis& bx) {
#pragma clang fp contract(off)
  return ((bx.b0 * p[0] + bx.b1 * p[1]) + bx.b2 * p[2]) + bx.b3 * p[3];
}

// Coordinates (in the scaled image) that crop pixel (cy, cx) of a warping sample reads, and from them the
// bilinear image value (rounded as a warp of a uint8 image) and the nearest mask value.  Contraction is off: the
// specification evaluates the same fp32 operations one by one in numpy.
DEVI void warp_sample(const AugSrc& s, const float* m, const float* lat, bool elastic, bool constant, int n,
                      float sy_scale, float sx_scale, int cy, int cx, int offy, int offx, float* rgb, uint8_t* mk) {
#pragma clang fp contract(off)
  const float fcy = (float)cy, fcx = (float)cx;
  float qy = (m[0] * fcy + m[1] * fcx) + m[2];
  float qx = (m[3] * fcy + m[4] * fcx) + m[5];
  if (elastic) {
    const float gy = fcy * sy_scale, gx = fcx * sx_scale;
    const int iy = min((int)floorf(gy), n - 1), ix = min((int)floorf(gx), n - 1);
    const Basis by = bspline_basis(gy - (float)iy), bx = bspline_basis(gx - (float)ix);
    const int ld = n + 3;
    const float* py = lat + iy * ld + ix;
    const float* px = py + kLattice;
    const float dy = ((by.b0 * bspline_row(py, bx) + by.b1 * bspline_row(py + ld, bx)) +
                      by.b2 * bspline_row(py + 2 * ld, bx)) + by.b3 * bspline_row(py + 3 * ld, bx);
    const float dx = ((by.b0 * bspline_row(px, bx) + by.b1 * bspline_row(px + ld, bx)) +
                      by.b2 * bspline_row(px + 2 * ld, bx)) + by.b3 * bspline_row(px + 3 * ld, bx);
    qy = qy + dy;
    qx = qx + dx;
  }
  const float fy = fminf(fmaxf(qy + (float)offy, -kCoordLimit), kCoordLimit);
  const float fx = fminf(fmaxf(qx + (float)offx, -kCoordLimit), kCoordLimit);
  const float y0f = floorf(fy), x0f = floorf(fx);
  const float ly = fy - y0f, lx = fx - x0f;
  const int y0 = (int)y0f, x0 = (int)x0f;
  float v00[3], v01[3], v10[3], v11[3];
  border_pixel(s, y0, x0, constant, v00);
  border_pixel(s, y0, x0 + 1, constant, v01);
  border_pixel(s, y0 + 1, x0, constant, v10);
  border_pixel(s, y0 + 1, x0 + 1, constant, v11);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = (1.f - ly) * ((1.f - lx) * v00[c] + lx * v01[c]) + ly * ((1.f - lx) * v10[c] + lx * v11[c]);
    rgb[c] = fminf(fmaxf(rintf(v), 0.f), 255.f);
  }
  const int my = (int)rintf(fy), mx = (int)rintf(fx);
  if (constant)
    *mk = (my < 0 || my >= s.nh || mx < 0 || mx >= s.nw) ? (uint8_t)0 : src_mask(s, my, mx);
  else
    *mk = src_mask(s, reflect101_any(my, s.nh), reflect101_any(mx, s.nw));
}

// aug_geometry for a batch in which at least one sample warps.  Grid (blocks per sample, B), one thread per
// output pixel; the block stages its sample's matrix and control lattice in LDS once.  A sample that does not
// warp takes the integer gather of aug_geometry_kernel.
__global__ __launch_bounds__(kBlock) void aug_warp_kernel(const uint8_t* __restrict__ images,
                                                          const uint8_t* __restrict__ masks,
                                                          const int64_t* __restrict__ meta,
                                                          const int* __restrict__ ip, const int* __restrict__ xi,
                                                          const float* __restrict__ xf, float* __restrict__ work,
                                                          int64_t* __restrict__ mask_out, int CH, int CW) {
  __shared__ float s_m[8];
  __shared__ float s_lat[2 * kLattice];
  const int b = blockIdx.y;
  const int* q = ip + b * kAugIParams;
  const int* e = xi + b * kAugXI;
  const float* f = xf + (long)b * kAugXF;
  const int flags = e[0];
  const bool warps = (flags & kAugWarp) != 0, elastic = warps && (flags & kAugElastic) != 0;
  const int n = min(max(e[1], 1), 8);
  if (warps) {
    if (threadIdx.x < 8) s_m[threadIdx.x] = f[threadIdx.x];
    if (elastic)
      for (int i = threadIdx.x; i < 2 * kLattice; i += kBlock) s_lat[i] = f[kXfLattice + i];
  }
  __syncthreads();
  const int pix = blockIdx.x * kBlock + threadIdx.x;
  if (pix >= CH * CW) return;
  const int oy = pix / CW, ox = pix - oy * CW;
  const int img = q[0];
  AugSrc s;
  s.img = images + meta[4 * img];
  s.msk = masks + meta[4 * img + 3];
  s.h = (int)meta[4 * img + 1];
  s.w = (int)meta[4 * img + 2];
  s.nh = q[1];
  s.nw = q[2];
  // flips act last: output (oy, ox) reads crop pixel (cy, cx)
  const int cy = q[8] ? CH - 1 - oy : oy;
  const int cx = q[7] ? CW - 1 - ox : ox;
  float rgb[3];
  uint8_t m;
  if (warps) {
    warp_sample(s, s_m, s_lat, elastic, (flags & kAugConstant) != 0, n, f[6], f[7], cy, cx, q[5] - q[3],
                q[6] - q[4], rgb, &m);
  } else {
    const int sy = reflect101(cy + q[5] - q[3], s.nh);
    const int sx = reflect101(cx + q[6] - q[4], s.nw);
    src_pixel(s, sy, sx, rgb);
    m = src_mask(s, sy, sx);
  }
  const long i = (long)b * CH * CW + pix;
  float* o = work + i * 3;
  o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2];
  mask_out[i] = m;
}

// Philox4x32-10 (Salmon et al., SC'11) in registers
DEVI void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* out) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

DEVI float philox_uniform(uint32_t k) { return ((float)k + 0.5f) * 2.3283064365386963e-10f; }   // (k + 0.5) 2^-32

// Gamma and / or Gaussian noise per pixel, for the samples whose flags ask for an op in `ops`; the work buffer is
// in the output frame, so the noise counter is the pixel's index there.
__global__ __launch_bounds__(kBlock) void aug_pointwise_kernel(float* __restrict__ work, const int* __restrict__ xi,
                                                               const float* __restrict__ xf, int B, int HW, int ops) {
  const long total = (long)B * HW;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long)gridDim.x * kBlock) {
    const int b = (int)(i / HW);
    const int flags = xi[b * kAugXI] & ops;
    if (!(flags & (kAugGamma | kAugNoise))) continue;
    const float* f = xf + (long)b * kAugXF;
    float* px = work + i * 3;
    float v[3] = {px[0], px[1], px[2]};
    if (flags & kAugGamma) {
      const float g = f[8];
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = clip255(255.f * powf(v[c] / 255.f, g));
    }
    if (flags & kAugNoise) {
      uint32_t r[4];
      philox4x32_10((uint32_t)(i - (long)b * HW), 0u, 0u, 0u, (uint32_t)xi[b * kAugXI + 3],
                    (uint32_t)xi[b * kAugXI + 4], r);
      const float two_pi = 6.2831854820251465f;
      const float r0 = sqrtf(-2.f * logf(philox_uniform(r[0]))), a0 = two_pi * philox_uniform(r[1]);
      const float r1 = sqrtf(-2.f * logf(philox_uniform(r[2]))), a1 = two_pi * philox_uniform(r[3]);
      const float std = f[9];
      v[0] = clip255(v[0] + r0 * cosf(a0) * std);
      v[1] = clip255(v[1] + r0 * sinf(a0) * std);
      v[2] = clip255(v[2] + r1 * cosf(a1) * std);
    }
    px[0] = v[0]; px[1] = v[1]; px[2] = v[2];
  }
}

// Separable Gaussian blur in one pass, out of place: a block stages its 32x32 tile plus a halo of r (reflect-101
// inside the crop) in LDS, blurs the rows into a second LDS tile and the columns from there to `out`.  Rows are
// handled as 3 * width interleaved floats, so consecutive lanes touch consecutive LDS banks.  Each output is
// w0 x[i] + sum_k w_k (x[i-k] + x[i+k]), k ascending.  Samples that are not blurred are copied through.
constexpr int kBlurTile = 32, kBlurMaxR = 8, kBlurSpan = kBlurTile + 2 * kBlurMaxR;

__global__ __launch_bounds__(kBlock) void aug_blur_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                          const int* __restrict__ xi, const float* __restrict__ xf,
                                                          int CH, int CW) {
  __shared__ float s_in[kBlurSpan][kBlurSpan * 3];
  __shared__ float s_h[kBlurSpan][kBlurTile * 3];
  __shared__ float s_w[kBlurMaxR + 1];
  const int b = blockIdx.z;
  const int ty0 = blockIdx.y * kBlurTile, tx0 = blockIdx.x * kBlurTile;
  const float* src = in + (long)b * CH * CW * 3;
  float* dst = out + (long)b * CH * CW * 3;
  const int row = kBlurTile * 3;                      // floats of one tile row
  const int wid = min(kBlurTile, CW - tx0) * 3;       // ... of which inside the crop
  if (!(xi[b * kAugXI] & kAugBlur)) {
    for (int idx = threadIdx.x; idx < kBlurTile * row; idx += kBlock) {
      const int ty = idx / row, j = idx - ty * row;
      if (ty0 + ty < CH && j < wid) {
        const long g = ((long)(ty0 + ty) * CW + tx0) * 3 + j;
        dst[g] = src[g];
      }
    }
    return;
  }
  const int r = min(max(xi[b * kAugXI + 2], 1), kBlurMaxR);
  const int span = kBlurTile + 2 * r;
  if (threadIdx.x <= kBlurMaxR) s_w[threadIdx.x] = xf[(long)b * kAugXF + 10 + threadIdx.x];
  for (int idx = threadIdx.x; idx < span * span; idx += kBlock) {
    const int ty = idx / span, tx = idx - ty * span;
    const int gy = reflect101_any(ty0 - r + ty, CH), gx = reflect101_any(tx0 - r + tx, CW);
    const float* p = src + ((long)gy * CW + gx) * 3;
    s_in[ty][tx * 3] = p[0];
    s_in[ty][tx * 3 + 1] = p[1];
    s_in[ty][tx * 3 + 2] = p[2];
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < span * row; idx += kBlock) {
    const int ty = idx / row, j = idx - ty * row;
    const float* c = &s_in[ty][j + 3 * r];
    float acc = s_w[0] * c[0];
    for (int k = 1; k <= r; ++k) acc += s_w[k] * (c[-3 * k] + c[3 * k]);
    s_h[ty][j] = acc;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < kBlurTile * row; idx += kBlock) {
    const int ty = idx / row, j = idx - ty * row;
    if (ty0 + ty >= CH || j >= wid) continue;
    float acc = s_w[0] * s_h[ty + r][j];
    for (int k = 1; k <= r; ++k) acc += s_w[k] * (s_h[ty + r - k][j] + s_h[ty + r + k][j]);
    dst[((long)(ty0 + ty) * CW + tx0) * 3 + j] = clip255(acc);
  }
}
}  // namespace

void aug_geometry(const uint8_t* images, const uint8_t* masks, const int64_t* meta, const int* ip, float* work,
                  int64_t* mask_out, int B, int CH, int CW, hipStream_t s) {
  hipLaunchKernelGGL(aug_geometry_kernel, dim3(grid_for((long)B * CH * CW)), dim3(kBlock), 0, s, images, masks, meta,
                     ip, work, mask_out, B, CH, CW);
}

int aug_gray_scratch_doubles(int B) { return B * kGraySlices; }

void aug_gray_mean(const float* work, float* mean, double* part, int B, int HW, hipStream_t s) {
  hipLaunchKernelGGL(aug_gray_partial_kernel, dim3(kGraySlices, B), dim3(kBlock), 0, s, work, part, HW);
  hipLaunchKernelGGL(aug_gray_final_kernel, dim3((B + kBlock - 1) / kBlock), dim3(kBlock), 0, s, part, mean, B, HW);
}

void aug_color(float* work, const int* ip, const float* fp, const float* mean, int B, int HW, int stage,
               hipStream_t s) {
  hipLaunchKernelGGL(aug_color_kernel, dim3(grid_for((long)B * HW)), dim3(kBlock), 0, s, work, ip, fp, mean, B, HW,
                     stage);
}

void aug_finalize(const float* work, const int* ip, float* out, int B, int HW, const float* mean3, const float* std3,
                  hipStream_t s) {
  hipLaunchKernelGGL(aug_finalize_kernel, dim3(grid_for((long)B * HW)), dim3(kBlock), 0, s, work, ip, out, B, HW,
                     mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
}

void aug_warp(const uint8_t* images, const uint8_t* masks, const int64_t* meta, const int* ip, const int* xi,
              const float* xf, float* work, int64_t* mask_out, int B, int CH, int CW, hipStream_t s) {
  hipLaunchKernelGGL(aug_warp_kernel, dim3((CH * CW + kBlock - 1) / kBlock, B), dim3(kBlock), 0, s, images, masks,
                     meta, ip, xi, xf, work, mask_out, CH, CW);
}

void aug_pointwise(float* work, const int* xi, const float* xf, int B, int HW, int ops, hipStream_t s) {
  hipLaunchKernelGGL(aug_pointwise_kernel, dim3(grid_for((long)B * HW)), dim3(kBlock), 0, s, work, xi, xf, B, HW,
                     ops);
}

void aug_blur(const float* in, float* out, const int* xi, const float* xf, int B, int CH, int CW, hipStream_t s) {
  hipLaunchKernelGGL(aug_blur_kernel, dim3((CW + kBlurTile - 1) / kBlurTile, (CH + kBlurTile - 1) / kBlurTile, B),
                     dim3(kBlock), 0, s, in, out, xi, xf, CH, CW);
}
