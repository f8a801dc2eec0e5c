// The pooling and residual-merge glue of StarGAN v2's ResBlk / AdainResBlk (core/model.py:23-120), NHWC fp32.
//   avgpool2   F.avg_pool2d(x, 2) (even H and W) and its backward
//   merge      out = (a + f(b)) * s with f = identity | avgpool2 (b at twice a's resolution) | nearest up2 (b at
//              half a's resolution): the block's "(shortcut + residual) / sqrt(2)" in one pass with the shortcut's
//              resampling folded in; the backward writes ga = s * g and gb = s * f^T(g) from one read of g
// Memory-bound streaming kernels: one thread per float4 of channels of the LOW-resolution side (a thread of a
// resampling kernel owns a whole 2x2 block), 64-bit element indices throughout (N*H*W*C of a batch of 436 x 1024
// frames passes 2^31).  H, W are always the dimensions of the low-resolution side.
#include "common.h"

namespace vst {

__device__ __forceinline__ float4 scale_f4(float4 v, float s) {
  return make_float4(v.x * s, v.y * s, v.z * s, v.w * s);
}

// float4 index i of the low-resolution tensor [N][H][W][C4] -> the float4 index of the top-left pixel of its
// 2x2 block in [N][2H][2W][C4]; the block's pixels are at + {0, C4, row, row + C4}, row = 2 W C4
__device__ __forceinline__ long blk_hi(long i, int H, int W, int C4) {
  const long c4 = i % C4, pix = i / C4;
  const long w = pix % W, h = (pix / W) % H, n = pix / ((long)H * W);
  return ((n * 2 * H + 2 * h) * 2 * W + 2 * w) * C4 + c4;
}

// the 2x2 sum in scan order (0,0), (0,1), (1,0), (1,1)
__device__ __forceinline__ float4 sum2x2(const float4* __restrict__ x, long hi, long row, int C4) {
  float4 a = x[hi];
  add_f4(a, x[hi + C4]);
  add_f4(a, x[hi + row]);
  add_f4(a, x[hi + row + C4]);
  return a;
}

__device__ __forceinline__ void store2x2(float4* __restrict__ y, long hi, long row, int C4, float4 v) {
  y[hi] = v;
  y[hi + C4] = v;
  y[hi + row] = v;
  y[hi + row + C4] = v;
}

// the pre-activation blocks' standalone activation (its backward is vst_act_bwd, from the output)
__global__ void act_fwd_k(const float4* __restrict__ x, float4* __restrict__ y, long total4, int act, float slope) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total4) return;
  const float4 v = x[i];
  y[i] = make_float4(apply_act(v.x, act, slope), apply_act(v.y, act, slope), apply_act(v.z, act, slope),
                     apply_act(v.w, act, slope));
}

// y [N][H][W] = mean of x's 2x2 blocks, x [N][2H][2W]
__global__ void avgpool2_fwd_k(const float4* __restrict__ x, float4* __restrict__ y, long total, int H, int W,
                               int C4) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  y[i] = scale_f4(sum2x2(x, blk_hi(i, H, W, C4), 2L * W * C4, C4), 0.25f);
}

// gx [N][2H][2W]: every pixel of a block gets gy / 4
__global__ void avgpool2_bwd_k(const float4* __restrict__ gy, float4* __restrict__ gx, long total, int H, int W,
                               int C4) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  store2x2(gx, blk_hi(i, H, W, C4), 2L * W * C4, C4, scale_f4(gy[i], 0.25f));
}

// MODE VST_MERGE_SAME: total = the float4s of a.  VST_MERGE_POOL: a, out [N][H][W], b [N][2H][2W], total = the
// float4s of a.  VST_MERGE_UP: a, out [N][2H][2W], b [N][H][W], total = the float4s of b.
template <int MODE>
__global__ void merge_fwd_k(const float4* __restrict__ a, const float4* __restrict__ b, float4* __restrict__ out,
                            long total, int H, int W, int C4, float s) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  if constexpr (MODE == VST_MERGE_SAME) {
    float4 v = a[i];
    add_f4(v, b[i]);
    out[i] = scale_f4(v, s);
  } else if constexpr (MODE == VST_MERGE_POOL) {
    float4 v = a[i];
    add_f4(v, scale_f4(sum2x2(b, blk_hi(i, H, W, C4), 2L * W * C4, C4), 0.25f));
    out[i] = scale_f4(v, s);
  } else {
    const long hi = blk_hi(i, H, W, C4), row = 2L * W * C4;
    const float4 u = b[i];
    const long off[4] = {0, C4, row, row + C4};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float4 v = a[hi + off[k]];
      add_f4(v, u);
      out[hi + off[k]] = scale_f4(v, s);
    }
  }
}

// ga = s * g (g's shape) and gb = s * f^T(g) (b's shape); the same thread layout as the forward
template <int MODE>
__global__ void merge_bwd_k(const float4* __restrict__ g, float4* __restrict__ ga, float4* __restrict__ gb,
                            long total, int H, int W, int C4, float s) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  if constexpr (MODE == VST_MERGE_SAME) {
    const float4 v = scale_f4(g[i], s);
    ga[i] = v;
    gb[i] = v;
  } else if constexpr (MODE == VST_MERGE_POOL) {
    const float4 v = scale_f4(g[i], s);
    ga[i] = v;
    store2x2(gb, blk_hi(i, H, W, C4), 2L * W * C4, C4, scale_f4(v, 0.25f));
  } else {
    const long hi = blk_hi(i, H, W, C4), row = 2L * W * C4;
    const long off[4] = {0, C4, row, row + C4};
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float4 v = g[hi + off[k]];
      ga[hi + off[k]] = scale_f4(v, s);
      add_f4(acc, v);
    }
    gb[i] = scale_f4(acc, s);
  }
}

}  // namespace vst

using namespace vst;

extern "C" int vst_act_fwd(const float* x, float* y, long n, int act, float slope, void* stream) {
  VST_REQUIRE(x && y && n > 0 && n % 4 == 0, "act_fwd: bad args (n %% 4 == 0)");
  hipLaunchKernelGGL(act_fwd_k, dim3(ceil_div(n / 4, 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const float4*>(x), reinterpret_cast<float4*>(y), n / 4, act, slope);
  return check_launch("act_fwd");
}

// H, W: the OUTPUT's (low-resolution) dimensions; x is [N][2H][2W][C]
extern "C" int vst_avgpool2_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream) {
  VST_REQUIRE(x && y && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "avgpool2_fwd: bad args (C %% 4 == 0)");
  const long total = (long)N * H * W * (C / 4);
  hipLaunchKernelGGL(avgpool2_fwd_k, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const float4*>(x), reinterpret_cast<float4*>(y), total, H, W, C / 4);
  return check_launch("avgpool2_fwd");
}

extern "C" int vst_avgpool2_bwd(const float* gy, float* gx, int N, int H, int W, int C, void* stream) {
  VST_REQUIRE(gy && gx && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "avgpool2_bwd: bad args (C %% 4 == 0)");
  const long total = (long)N * H * W * (C / 4);
  hipLaunchKernelGGL(avgpool2_bwd_k, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const float4*>(gy), reinterpret_cast<float4*>(gx), total, H, W, C / 4);
  return check_launch("avgpool2_bwd");
}

static int merge_args(const char* what, bool ptrs, int N, int H, int W, int C, int mode) {
  VST_REQUIRE(ptrs && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "%s: bad args (C %% 4 == 0)", what);
  VST_REQUIRE(mode == VST_MERGE_SAME || mode == VST_MERGE_POOL || mode == VST_MERGE_UP, "%s: unknown mode %d", what,
              mode);
  return VST_OK;
}

// H, W: the dimensions of the low-resolution side (both sides' for VST_MERGE_SAME)
extern "C" int vst_merge_fwd(const float* a, const float* b, float* out, int N, int H, int W, int C, int mode,
                             float scale, void* stream) {
  if (const int rc = merge_args("merge_fwd", a && b && out, N, H, W, C, mode)) return rc;
  const long total = (long)N * H * W * (C / 4);
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(a), reinterpret_cast<const float4*>(b),
                       reinterpret_cast<float4*>(out), total, H, W, C / 4, scale);
  };
  if (mode == VST_MERGE_SAME) launch(merge_fwd_k<VST_MERGE_SAME>);
  else if (mode == VST_MERGE_POOL) launch(merge_fwd_k<VST_MERGE_POOL>);
  else launch(merge_fwd_k<VST_MERGE_UP>);
  return check_launch("merge_fwd");
}

extern "C" int vst_merge_bwd(const float* g, float* ga, float* gb, int N, int H, int W, int C, int mode, float scale,
                             void* stream) {
  if (const int rc = merge_args("merge_bwd", g && ga && gb, N, H, W, C, mode)) return rc;
  const long total = (long)N * H * W * (C / 4);
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(g), reinterpret_cast<float4*>(ga),
                       reinterpret_cast<float4*>(gb), total, H, W, C / 4, scale);
  };
  if (mode == VST_MERGE_SAME) launch(merge_bwd_k<VST_MERGE_SAME>);
  else if (mode == VST_MERGE_POOL) launch(merge_bwd_k<VST_MERGE_POOL>);
  else launch(merge_bwd_k<VST_MERGE_UP>);
  return check_launch("merge_bwd");
}
