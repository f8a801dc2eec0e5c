// Temporal losses of the learning-based video methods and the plane resize that feeds them.
//
// temporal_sq_k: methods/learning-based/fs_huang.py:55-56 (output temporal loss), fs_reconet.py:61-69
// (feature-map temporal loss; output temporal loss with the luminance-weighted input term) as ONE pass
// per direction over NHWC fp32 tensors:
//   L = scale / (N*Cl*H*W) * sum_{n,h,w,c<Cl} (m[n,h,w] * (s*b[n,h,w,c] - warp_m(s*a, flow)[n,h,w,c] - r[n,h,w]))^2
// with warp_m = fs_lib.warp (fs_lib.py:5-39: grid_sample * validity mask, bilin.h), s = ab_scale (the
// reference divides the net's 0..255 output by 255 before it takes the loss) and r = 0 or the input term
//   r = 0.2126 d0 + 0.7152 d1 + 0.0722 d2,  d = i2 - warp_m(i1, flow)          (fs_reconet.py:66-67)
// taken from the two input frames with the same sample geometry, so it costs no pass of its own.
// Threads are (pixel, float4 channel chunk) as in flow.hip's warp_fwd_k: the lanes of a pixel read its
// flow and mask once and gather each corner as contiguous float4s, so a 128-channel feature map moves as
// 512-byte rows.  Bytes per direction (fp32): forward a (gathered, <= 4 corners from cache) + b once;
// backward the same reads + gb written once + ga's atomic adds.
// resize_bilinear_k: F.interpolate(mode='bilinear', align_corners=False) of the NCHW flow / mask planes
// (fs_reconet.py:57-60) with a per-channel multiplier (the flow rescale of :58-59).
#include "common.h"

// Sample geometry, validity and the bilinear sum round as flow.hip's warp does (see there).
#pragma clang fp contract(off)
#include "bilin.h"

namespace vst {

// Four corner float4s of an NHWC image (C4 float4s per pixel) at chunk c4, zeros outside the frame.
struct Corners {
  float4 nw, ne, sw, se;
};

__device__ __forceinline__ Corners gather_corners(const float4* __restrict__ xs, const Bilin& b, int H, int W,
                                                  int C4) {
  Corners c;
  c.nw = c.ne = c.sw = c.se = make_float4(0.f, 0.f, 0.f, 0.f);
  const int r0 = b.y0 * W, r1 = r0 + W;
  if (inb(b.y0, b.x0, H, W)) c.nw = xs[(long)(r0 + b.x0) * C4];
  if (inb(b.y0, b.x0 + 1, H, W)) c.ne = xs[(long)(r0 + b.x0 + 1) * C4];
  if (inb(b.y0 + 1, b.x0, H, W)) c.sw = xs[(long)(r1 + b.x0) * C4];
  if (inb(b.y0 + 1, b.x0 + 1, H, W)) c.se = xs[(long)(r1 + b.x0 + 1) * C4];
  return c;
}

__device__ __forceinline__ float4 scale4(const float4& v, float s) {
  return make_float4(v.x * s, v.y * s, v.z * s, v.w * s);
}

// bilinear sample of the (already scaled) corners
__device__ __forceinline__ float4 bilerp4(const Corners& c, const Bilin& b) {
  float4 o;
  o.x = bilerp(c.nw.x, c.ne.x, c.sw.x, c.se.x, b.nw, b.ne, b.sw, b.se);
  o.y = bilerp(c.nw.y, c.ne.y, c.sw.y, c.se.y, b.nw, b.ne, b.sw, b.se);
  o.z = bilerp(c.nw.z, c.ne.z, c.sw.z, c.se.z, b.nw, b.ne, b.sw, b.se);
  o.w = bilerp(c.nw.w, c.ne.w, c.sw.w, c.se.w, b.nw, b.ne, b.sw, b.se);
  return o;
}

// Grid (ceil(W*C4 / 256), H, N).  part != NULL: the block's sum of e^2 as one double (forward);
// gout != NULL: gb = k * m * e written (channels >= Cl zero), ga += scatter(-w_corner * gb) through valid
// samples (ga may be NULL: the deterministic route takes ga from gb), k = kscale * gout[0].
// RTERM: the input term from i1, i2 (NHWC4; C4 == 1).  CT: C4 at compile time, 0 = runtime.
template <int RTERM, int CT>
__global__ __launch_bounds__(256) void temporal_sq_k(
    const float* __restrict__ a, const float* __restrict__ bimg, const float* __restrict__ flow,
    const float* __restrict__ mask, const float* __restrict__ i1, const float* __restrict__ i2,
    double* __restrict__ part, float* __restrict__ ga, float* __restrict__ gb, const float* __restrict__ gout,
    float kscale, float ab_scale, int N, int H, int W, int C4_, int Cl) {
  __shared__ double red[4];
  const int C4 = CT ? CT : C4_;
  const int local = blockIdx.x * 256 + threadIdx.x;
  const int h = blockIdx.y, n = blockIdx.z;
  double acc = 0.0;
  if (local < W * C4) {
    const int w = CT == 1 ? local : local / C4, c4 = CT == 1 ? 0 : local - w * C4;
    const long plane = (long)H * W;
    const long fo = (long)n * 2 * plane + (long)h * W + w;
    const Bilin b = bilin(h, w, flow[fo], flow[fo + plane], H, W, 0);
    const bool valid = warp_valid(b, H, W);
    const float m = mask[(long)n * plane + (long)h * W + w];
    const long po = ((long)n * plane + (long)h * W) * C4 + local;  // this thread's float4 of b / gb
    float4 wv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (valid) {
      Corners c = gather_corners(reinterpret_cast<const float4*>(a) + (long)n * plane * C4 + c4, b, H, W, C4);
      c.nw = scale4(c.nw, ab_scale);
      c.ne = scale4(c.ne, ab_scale);
      c.sw = scale4(c.sw, ab_scale);
      c.se = scale4(c.se, ab_scale);
      wv = bilerp4(c, b);
    }
    float r = 0.f;
    if (RTERM) {
      float4 wi = make_float4(0.f, 0.f, 0.f, 0.f);
      if (valid) wi = bilerp4(gather_corners(reinterpret_cast<const float4*>(i1) + (long)n * plane, b, H, W, 1), b);
      const float4 t = reinterpret_cast<const float4*>(i2)[po];
      r = 0.2126f * (t.x - wi.x) + 0.7152f * (t.y - wi.y) + 0.0722f * (t.z - wi.z);
    }
    const float4 bv = scale4(reinterpret_cast<const float4*>(bimg)[po], ab_scale);
    const int nl = Cl - c4 * 4;  // logical channels of this chunk (>= 4: all)
    float4 e;
    e.x = nl > 0 ? m * (bv.x - wv.x - r) : 0.f;
    e.y = nl > 1 ? m * (bv.y - wv.y - r) : 0.f;
    e.z = nl > 2 ? m * (bv.z - wv.z - r) : 0.f;
    e.w = nl > 3 ? m * (bv.w - wv.w - r) : 0.f;
    acc = (double)(e.x * e.x) + (double)(e.y * e.y) + (double)(e.z * e.z) + (double)(e.w * e.w);
    if (gout) {
      const float k = kscale * gout[0] * m;
      const float4 g = make_float4(k * e.x, k * e.y, k * e.z, k * e.w);
      if (gb) reinterpret_cast<float4*>(gb)[po] = g;
      if (CT >= 4 && CT % 4 == 0) {
        // Wide pixels: transpose gb within the pixel's CT lanes so that lane c4 holds channels CT*j + c4
        // (j = 0..3): each atomic wave-instruction then covers CT contiguous floats per pixel (two 128-byte
        // segments per wave at CT = 32) instead of 4-byte pieces 16 bytes apart.  A pixel's lanes share its
        // flow, so they are all here or all not (256 and 64 are multiples of CT).
        const int grp = (threadIdx.x & 63) - c4;
        float t[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int src = grp + (CT / 4) * j + (c4 >> 2);
          const float tx = __shfl(g.x, src, 64), ty = __shfl(g.y, src, 64);
          const float tz = __shfl(g.z, src, 64), tw = __shfl(g.w, src, 64);
          const int k4 = c4 & 3;
          t[j] = k4 == 0 ? tx : k4 == 1 ? ty : k4 == 2 ? tz : tw;
        }
        if (ga && valid) {
          float* base = ga + (long)n * plane * C4 * 4 + c4;
          for_corners(b, H, W, [&](int y, int xx, float wt) {
            float* d = base + ((long)y * W + xx) * C4 * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (CT * j + c4 < Cl) atomicAdd(d + CT * j, -wt * t[j]);
          });
        }
      } else if (ga && valid) {
        float* base = ga + ((long)n * plane * C4 + c4) * 4;
        for_corners(b, H, W, [&](int y, int xx, float wt) {
          float* d = base + ((long)y * W + xx) * C4 * 4;
          atomicAdd(d, -wt * g.x);
          if (nl > 1) atomicAdd(d + 1, -wt * g.y);
          if (nl > 2) atomicAdd(d + 2, -wt * g.z);
          if (nl > 3) atomicAdd(d + 3, -wt * g.w);
        });
      }
    }
  }
  if (part) {
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0)
      part[((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

// fixed-order final reduction of the per-block doubles: out[0] = scale * sum(part[0..n))
__global__ void finish_sum_d_k(const double* __restrict__ part, int n, float* __restrict__ out, double scale) {
  __shared__ double red[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += part[i];
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (float)(((red[0] + red[1]) + (red[2] + red[3])) * scale);
}

static dim3 temporal_grid(int N, int H, int W, int Cs) { return dim3(ceil_div((long)W * (Cs / 4), 256), H, N); }

static void temporal_sq_launch(const float* a, const float* b, const float* flow, const float* mask, const float* i1,
                               const float* i2, double* part, float* ga, float* gb, const float* gout, float kscale,
                               float ab_scale, int N, int H, int W, int Cs, int Cl, hipStream_t s) {
  const int C4 = Cs / 4;
  const dim3 grid = temporal_grid(N, H, W, Cs);
#define VST_TSQ(R, CT)                                                                                          \
  hipLaunchKernelGGL((temporal_sq_k<R, CT>), grid, dim3(256), 0, s, a, b, flow, mask, i1, i2, part, ga, gb, gout, \
                     kscale, ab_scale, N, H, W, C4, Cl)
  if (i1) VST_TSQ(1, 1);
  else if (C4 == 1) VST_TSQ(0, 1);
  else if (C4 == 16) VST_TSQ(0, 16);
  else if (C4 == 32) VST_TSQ(0, 32);
  else VST_TSQ(0, 0);
#undef VST_TSQ
}

// y[n][c][oy][ox] = mult[c] * bilinear(x[n][c]) at the source position (o + 0.5) * (in / out) - 0.5 clamped at
// 0, neighbours clamped at the last row / column: ATen's upsample_bilinear2d (align_corners=False, no antialias).
__global__ void resize_bilinear_k(const float* __restrict__ x, const float* __restrict__ mult, float* __restrict__ y,
                                  long total, int C, int Hi, int Wi, int Ho, int Wo, float sh, float sw) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int ox = i % Wo, oy = (i / Wo) % Ho;
  const long nc = i / ((long)Wo * Ho);
  float fy = sh * ((float)oy + 0.5f) - 0.5f, fx = sw * ((float)ox + 0.5f) - 0.5f;
  fy = fy < 0.f ? 0.f : fy;
  fx = fx < 0.f ? 0.f : fx;
  const int y0 = min((int)fy, Hi - 1), x0 = min((int)fx, Wi - 1);
  const int y1 = y0 + (y0 < Hi - 1 ? 1 : 0), x1 = x0 + (x0 < Wi - 1 ? 1 : 0);
  const float ly = fy - (float)y0, lx = fx - (float)x0;
  const float hy = 1.f - ly, hx = 1.f - lx;
  const float* p = x + nc * (long)Hi * Wi;
  const float top = hx * p[(long)y0 * Wi + x0] + lx * p[(long)y0 * Wi + x1];
  const float bot = hx * p[(long)y1 * Wi + x0] + lx * p[(long)y1 * Wi + x1];
  const float v = hy * top + ly * bot;
  y[i] = mult ? v * mult[nc % C] : v;
}

}  // namespace vst

using namespace vst;

// one double per block of temporal_sq_k, in floats, + alignment slack
extern "C" int vst_temporal_sqdiff_part_floats(int N, int H, int W, int Cs) {
  if (N <= 0 || H <= 0 || W <= 0 || Cs < 4) return 0;
  return 2 * ceil_div((long)W * (Cs / 4), 256) * H * N + 2;
}

static int temporal_sq_check(const char* what, int N, int H, int W, int Cs, int Cl, const float* i1,
                             const float* i2) {
  VST_REQUIRE(N > 0 && H > 0 && W > 0 && Cs > 0 && Cs % 4 == 0 && Cl > 0 && Cl <= Cs, "%s: bad args", what);
  VST_REQUIRE((i1 != nullptr) == (i2 != nullptr), "%s: the input term needs both frames", what);
  VST_REQUIRE(!i1 || (Cs == 4 && Cl == 3), "%s: the input term is for NHWC4 frames (Cs 4, Cl 3)", what);
  VST_REQUIRE(Cl > Cs - 4, "%s: only the last channel chunk may hold padding (Cl > Cs - 4)", what);
  VST_REQUIRE(H <= 65535 && N <= 65535 && (long)W * (Cs / 4) < (1L << 31) &&
                  (long)ceil_div((long)W * (Cs / 4), 256) * H * N < (1L << 30),
              "%s: grid too large", what);
  return VST_OK;
}

extern "C" int vst_temporal_sqdiff_fwd(const float* a, const float* b, const float* flow, const float* mask,
                                       const float* i1, const float* i2, float* loss, float* part, int N, int H,
                                       int W, int Cs, int Cl, float scale, float ab_scale, void* stream) {
  VST_REQUIRE(a && b && flow && mask && loss && part, "temporal_sqdiff_fwd: bad args");
  if (int e = temporal_sq_check("temporal_sqdiff_fwd", N, H, W, Cs, Cl, i1, i2)) return e;
  hipStream_t s = (hipStream_t)stream;
  double* pd = reinterpret_cast<double*>(((uintptr_t)part + 7) & ~(uintptr_t)7);
  const dim3 grid = temporal_grid(N, H, W, Cs);
  const int nb = (int)((long)grid.x * grid.y * grid.z);
  temporal_sq_launch(a, b, flow, mask, i1, i2, pd, nullptr, nullptr, nullptr, 0.f, ab_scale, N, H, W, Cs, Cl, s);
  hipLaunchKernelGGL(finish_sum_d_k, dim3(1), dim3(256), 0, s, pd, nb, loss,
                     (double)scale / ((double)N * H * W * Cl));
  return check_launch("temporal_sqdiff_fwd");
}

extern "C" int vst_temporal_sqdiff_bwd(const float* a, const float* b, const float* flow, const float* mask,
                                       const float* i1, const float* i2, const float* gout, float* ga, float* gb,
                                       int N, int H, int W, int Cs, int Cl, float scale, float ab_scale,
                                       void* stream) {
  VST_REQUIRE(a && b && flow && mask && gout && (ga || gb), "temporal_sqdiff_bwd: bad args");
  if (int e = temporal_sq_check("temporal_sqdiff_bwd", N, H, W, Cs, Cl, i1, i2)) return e;
  // d/d(s*b) = 2 * scale / count * m * e; the chain through the load scale s folds into k
  const float k = (float)(2.0 * scale * ab_scale / ((double)N * H * W * Cl));
  temporal_sq_launch(a, b, flow, mask, i1, i2, nullptr, ga, gb, gout, k, ab_scale, N, H, W, Cs, Cl,
                     (hipStream_t)stream);
  return check_launch("temporal_sqdiff_bwd");
}

extern "C" int vst_resize_bilinear(const float* x, const float* mult, float* y, int N, int C, int Hi, int Wi,
                                   int Ho, int Wo, void* stream) {
  VST_REQUIRE(x && y && N > 0 && C > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0, "resize_bilinear: bad args");
  const long total = (long)N * C * Ho * Wo;
  VST_REQUIRE(total < (1L << 31) * 256, "resize_bilinear: grid too large");
  hipLaunchKernelGGL(resize_bilinear_k, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, x, mult, y,
                     total, C, Hi, Wi, Ho, Wo, (float)Hi / (float)Ho, (float)Wi / (float)Wo);
  return check_launch("resize_bilinear");
}
