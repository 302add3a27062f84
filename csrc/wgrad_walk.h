// The weight-gradient GEMM's pixel cursor (conv_wgrad_gemm.hip), host and device: the kernel steps its X addresses
// with these functions and bindings.cpp traces them on the host (wgrad_cursor_trace, tests/test_wgrad_cursor_cpu.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The weight-gradient GEMM's pixel cursor: a lane's walk over output pixels m0, m0 + step, m0 + 2 step, ... kept as
// (n, oh*stride, ow*stride, base) with base = (n*IH + oh*stride)*IW + ow*stride, the input pixel index before the
// tap offset.  The step is uniform and decomposed once on the host (dow = step % OW, doh = (step / OW) % OH,
// dn = step / (OH*OW)), so an advance is adds and two carries: no division, no multiply.  One function for the
// kernel and for the host trace the CPU test compares with divmod (wgrad_cursor_trace).
struct WgWalk {
  int N, IH, IW;
  int ows_lim, ohs_lim;   // OW*stride, OH*stride
  int stride;
  int dows, dohs, dn;     // the step, (ow, oh) parts scaled by the stride
  uint32_t dbase;         // base's share of the step: dows + dohs*IW + dn*IH*IW
  uint32_t wrap_w;        // ... of an ow carry: stride*IW - OW*stride   (mod 2^32)
  uint32_t wrap_h;        // ... of an oh carry: IH*IW - OH*stride*IW    (mod 2^32)
};
struct WgCursor { int n, ohs, ows; uint32_t base; };

__host__ __device__ inline WgWalk wg_walk_make(int N, int IH, int IW, int OH, int OW, int stride, int step) {
  WgWalk w;
  w.N = N; w.IH = IH; w.IW = IW; w.stride = stride;
  w.ows_lim = OW * stride; w.ohs_lim = OH * stride;
  w.dows = (step % OW) * stride;
  w.dohs = ((step / OW) % OH) * stride;
  w.dn = step / (OH * OW);
  w.dbase = (uint32_t)w.dows + (uint32_t)w.dohs * (uint32_t)IW + (uint32_t)w.dn * (uint32_t)(IH * IW);
  w.wrap_w = (uint32_t)(stride * IW) - (uint32_t)(OW * stride);
  w.wrap_h = (uint32_t)(IH * IW) - (uint32_t)(OH * stride) * (uint32_t)IW;
  return w;
}
// the cursor at output pixel (n, oh, ow)
__host__ __device__ inline WgCursor wg_cursor_init(const WgWalk& w, int n, int oh, int ow) {
  WgCursor c;
  c.n = n; c.ohs = oh * w.stride; c.ows = ow * w.stride;
  c.base = ((uint32_t)n * (uint32_t)w.IH + (uint32_t)c.ohs) * (uint32_t)w.IW + (uint32_t)c.ows;
  return c;
}
// one step on (ow + dow < 2 OW and oh + doh + 1 < 2 OH: one carry each)
__host__ __device__ inline void wg_cursor_advance(const WgWalk& w, WgCursor& c) {
  c.ows += w.dows;
  c.base += w.dbase;
  const bool cw = c.ows >= w.ows_lim;
  c.ows -= cw ? w.ows_lim : 0;
  c.ohs += w.dohs + (cw ? w.stride : 0);
  c.base += cw ? w.wrap_w : 0u;
  const bool ch = c.ohs >= w.ohs_lim;
  c.ohs -= ch ? w.ohs_lim : 0;
  c.n += w.dn + (ch ? 1 : 0);
  c.base += ch ? w.wrap_h : 0u;
}
// tap (dy, dx) of the cursor's pixel: inside the batch and the image?  (its input pixel index is
// base + dy*IW + dx, meaningful only then)
__host__ __device__ inline bool wg_cursor_in(const WgWalk& w, const WgCursor& c, int dy, int dx) {
  return (int)(c.n < w.N) & (int)((unsigned)(c.ohs + dy) < (unsigned)w.IH) & (int)((unsigned)(c.ows + dx) < (unsigned)w.IW);
}
