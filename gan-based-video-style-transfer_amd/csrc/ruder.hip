// The recurrence glue of the Ruder video method (methods/learning-based/fs_ruder.py:38-108): frame k is styled
// from the 7-channel input cat(frame_k, mask_{k-1}, fs_lib.warp(styled_{k-1} / 255, flow_{k-1})), the loss is
// taken on the last frame and its gradient runs back through every warp.
//
// ruder_stack_k:     builds the net's next input in one pass.  Per pixel: img (float4), mask, flow (2 floats)
//                    and <= 4 corner float4s of y_prev (gathered, from cache) in; x (2 float4s: img rgb, mask |
//                    warp rgb, 0) and w (1 float4: the same warp, pad 0) out: 16 + 12 + <= 64 bytes read, 48
//                    bytes written per pixel.  Blank form (fs_ruder.py:78, no previous frame): 16 bytes read,
//                    48 written (32 when w is not asked for).
// ruder_temporal_k:  the temporal loss of fs_ruder.py:97 on the tensors the recurrence already holds (w from the
//                    last stack, y the last styled frame): no second gather.
//                      L = scale / (N*3*H*W) * sum_{c<3} (m * (w_c - s*y_c))^2
//                    Forward 16 + 16 + 4 bytes read per pixel, one double per block written; backward the same
//                    reads + gw and gy written (16 bytes each, pad channel 0).
// ruder_stack_bwd_k: the one scatter of the recurrence, gy_prev += s * scatter(corner weights * (gx[4..6] + gw))
//                    through valid samples: 16 (gx's upper float4) + 16 (gw) + 8 (flow) bytes read per pixel and
//                    <= 12 atomic adds; or the combined, s-scaled gradient written as NHWC4 (16 bytes) for the
//                    ordered scatter of flow_det.hip (ops.set_deterministic).
// One thread per pixel (the channel counts are 4 and 8); every image access is a float4.
#include "common.h"

// Sample geometry, validity and the bilinear sum round as flow.hip's warp does (see there).
#pragma clang fp contract(off)
#include "bilin.h"

namespace vst {

// y_prev == NULL: the blank form (flow, mask unused).  w may be NULL.
__global__ __launch_bounds__(256) void ruder_stack_k(const float4* __restrict__ y_prev, const float4* __restrict__ img,
                                                     const float* __restrict__ flow, const float* __restrict__ mask,
                                                     float4* __restrict__ x, float4* __restrict__ wout, int N, int H,
                                                     int W, float s) {
  const long plane = (long)H * W, total = (long)N * plane;
  const long pix = (long)blockIdx.x * 256 + threadIdx.x;
  if (pix >= total) return;
  float4 lo = img[pix];
  float4 hi = make_float4(0.f, 0.f, 0.f, 0.f);
  lo.w = 0.f;
  if (y_prev) {
    const int n = (int)(pix / plane);
    const long r = pix - (long)n * plane;
    const int h = (int)(r / W), w = (int)(r - (long)h * W);
    const long fo = (long)n * 2 * plane + r;
    const Bilin b = bilin(h, w, flow[fo], flow[fo + plane], H, W, 0);
    lo.w = mask[pix];
    if (warp_valid(b, H, W)) {
      const float4* ys = y_prev + (long)n * plane;
      float4 nw = hi, ne = hi, sw = hi, se = hi;
      const int r0 = b.y0 * W, r1 = r0 + W;
      if (inb(b.y0, b.x0, H, W)) nw = ys[r0 + b.x0];
      if (inb(b.y0, b.x0 + 1, H, W)) ne = ys[r0 + b.x0 + 1];
      if (inb(b.y0 + 1, b.x0, H, W)) sw = ys[r1 + b.x0];
      if (inb(b.y0 + 1, b.x0 + 1, H, W)) se = ys[r1 + b.x0 + 1];
      // the reference divides the styled frame by 255 before it warps: scale the corners, then sample
      hi.x = bilerp(nw.x * s, ne.x * s, sw.x * s, se.x * s, b.nw, b.ne, b.sw, b.se);
      hi.y = bilerp(nw.y * s, ne.y * s, sw.y * s, se.y * s, b.nw, b.ne, b.sw, b.se);
      hi.z = bilerp(nw.z * s, ne.z * s, sw.z * s, se.z * s, b.nw, b.ne, b.sw, b.se);
    }
  }
  x[pix * 2] = lo;
  x[pix * 2 + 1] = hi;
  if (wout) wout[pix] = hi;
}

// part != NULL: the block's sum of e^2 as one double (forward).  gout != NULL: gw = k * m * e, gy = -s * gw
// (either may be NULL), k = kscale * gout[0]; pad channels 0.
__global__ __launch_bounds__(256) void ruder_temporal_k(const float4* __restrict__ wimg, const float4* __restrict__ y,
                                                        const float* __restrict__ mask, double* __restrict__ part,
                                                        float4* __restrict__ gw, float4* __restrict__ gy,
                                                        const float* __restrict__ gout, float kscale, float s,
                                                        long total) {
  __shared__ double red[4];
  const long pix = (long)blockIdx.x * 256 + threadIdx.x;
  double acc = 0.0;
  if (pix < total) {
    const float4 wv = wimg[pix], yv = y[pix];
    const float m = mask[pix];
    const float ex = m * (wv.x - yv.x * s), ey = m * (wv.y - yv.y * s), ez = m * (wv.z - yv.z * s);
    acc = (double)(ex * ex) + (double)(ey * ey) + (double)(ez * ez);
    if (gout) {
      const float k = kscale * gout[0] * m;
      const float4 g = make_float4(k * ex, k * ey, k * ez, 0.f);
      if (gw) gw[pix] = g;
      if (gy) gy[pix] = make_float4(-s * g.x, -s * g.y, -s * g.z, 0.f);
    }
  }
  if (part) {
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

// fixed-order final reduction of the per-block doubles (temporal.hip's finish_sum_d_k)
__global__ void ruder_finish_sum_d_k(const double* __restrict__ part, int n, float* __restrict__ out, double scale) {
  __shared__ double red[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += part[i];
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (float)(((red[0] + red[1]) + (red[2] + red[3])) * scale);
}

// g = s * (gx[4..6] + gw) (either NULL = 0).  gbuf != NULL: g written as NHWC4 (pad 0, valid or not: the ordered
// scatter applies the validity).  gy_prev != NULL: gy_prev += scatter(corner weight * g) through valid samples.
__global__ __launch_bounds__(256) void ruder_stack_bwd_k(const float4* __restrict__ gx, const float4* __restrict__ gw,
                                                         const float* __restrict__ flow, float* __restrict__ gy_prev,
                                                         float4* __restrict__ gbuf, int N, int H, int W, float s) {
  const long plane = (long)H * W, total = (long)N * plane;
  const long pix = (long)blockIdx.x * 256 + threadIdx.x;
  if (pix >= total) return;
  float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
  if (gx) g = gx[pix * 2 + 1];
  if (gw) {
    const float4 t = gw[pix];
    g.x += t.x;
    g.y += t.y;
    g.z += t.z;
  }
  g = make_float4(s * g.x, s * g.y, s * g.z, 0.f);
  if (gbuf) gbuf[pix] = g;
  if (!gy_prev) return;
  const int n = (int)(pix / plane);
  const long r = pix - (long)n * plane;
  const int h = (int)(r / W), w = (int)(r - (long)h * W);
  const long fo = (long)n * 2 * plane + r;
  const Bilin b = bilin(h, w, flow[fo], flow[fo + plane], H, W, 0);
  if (!warp_valid(b, H, W)) return;
  float* base = gy_prev + (long)n * plane * 4;
  for_corners(b, H, W, [&](int yy, int xx, float wt) {
    float* d = base + ((long)yy * W + xx) * 4;
    atomicAdd(d, wt * g.x);
    atomicAdd(d + 1, wt * g.y);
    atomicAdd(d + 2, wt * g.z);
  });
}

static int ruder_shape_check(const char* what, int N, int H, int W) {
  VST_REQUIRE(N > 0 && H > 0 && W > 0, "%s: bad args (N, H, W >= 1)", what);
  VST_REQUIRE((long)N * H * W < (1L << 31), "%s: frame batch too large", what);
  return VST_OK;
}

}  // namespace vst

using namespace vst;

extern "C" int vst_ruder_stack_fwd(const float* y_prev, const float* img, const float* flow, const float* mask,
                                   float* x, float* w, int N, int H, int W, float s, void* stream) {
  VST_REQUIRE(img && x, "ruder_stack_fwd: bad args");
  VST_REQUIRE((y_prev != nullptr) == (flow != nullptr) && (y_prev != nullptr) == (mask != nullptr),
              "ruder_stack_fwd: bad args (y_prev, flow and mask are given together or all NULL)");
  if (int e = ruder_shape_check("ruder_stack_fwd", N, H, W)) return e;
  const long total = (long)N * H * W;
  hipLaunchKernelGGL(ruder_stack_k, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const float4*>(y_prev), reinterpret_cast<const float4*>(img), flow, mask,
                     reinterpret_cast<float4*>(x), reinterpret_cast<float4*>(w), N, H, W, s);
  return check_launch("ruder_stack_fwd");
}

extern "C" int vst_ruder_stack_bwd(const float* gx, const float* gw, const float* flow, float* gy_prev, float* gbuf,
                                   int N, int H, int W, float s, void* stream) {
  VST_REQUIRE((gx || gw) && flow && (gy_prev || gbuf), "ruder_stack_bwd: bad args");
  if (int e = ruder_shape_check("ruder_stack_bwd", N, H, W)) return e;
  const long total = (long)N * H * W;
  hipLaunchKernelGGL(ruder_stack_bwd_k, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const float4*>(gx), reinterpret_cast<const float4*>(gw), flow, gy_prev,
                     reinterpret_cast<float4*>(gbuf), N, H, W, s);
  return check_launch("ruder_stack_bwd");
}

// one double per block of ruder_temporal_k, in floats, + alignment slack
extern "C" int vst_ruder_temporal_part_floats(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0 || (long)N * H * W >= (1L << 31)) return 0;
  return 2 * ceil_div((long)N * H * W, 256) + 2;
}

extern "C" int vst_ruder_temporal_fwd(const float* w, const float* y, const float* mask, float* loss, float* part,
                                      int N, int H, int W, float scale, float s, void* stream) {
  VST_REQUIRE(w && y && mask && loss && part, "ruder_temporal_fwd: bad args");
  if (int e = ruder_shape_check("ruder_temporal_fwd", N, H, W)) return e;
  hipStream_t st = (hipStream_t)stream;
  const long total = (long)N * H * W;
  const int nb = ceil_div(total, 256);
  double* pd = reinterpret_cast<double*>(((uintptr_t)part + 7) & ~(uintptr_t)7);
  hipLaunchKernelGGL(ruder_temporal_k, dim3(nb), dim3(256), 0, st, reinterpret_cast<const float4*>(w),
                     reinterpret_cast<const float4*>(y), mask, pd, (float4*)nullptr, (float4*)nullptr,
                     (const float*)nullptr, 0.f, s, total);
  hipLaunchKernelGGL(ruder_finish_sum_d_k, dim3(1), dim3(256), 0, st, pd, nb, loss,
                     (double)scale / ((double)total * 3.0));
  return check_launch("ruder_temporal_fwd");
}

extern "C" int vst_ruder_temporal_bwd(const float* w, const float* y, const float* mask, const float* gout, float* gw,
                                      float* gy, int N, int H, int W, float scale, float s, void* stream) {
  VST_REQUIRE(w && y && mask && gout && (gw || gy), "ruder_temporal_bwd: bad args");
  if (int e = ruder_shape_check("ruder_temporal_bwd", N, H, W)) return e;
  const long total = (long)N * H * W;
  const float k = (float)(2.0 * scale / ((double)total * 3.0));
  hipLaunchKernelGGL(ruder_temporal_k, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const float4*>(w), reinterpret_cast<const float4*>(y), mask, (double*)nullptr,
                     reinterpret_cast<float4*>(gw), reinterpret_cast<float4*>(gy), gout, k, s, total);
  return check_launch("ruder_temporal_bwd");
}
