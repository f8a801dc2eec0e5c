// The two losses of StarGAN v2's discriminator update (StarGANv2AdvCon core/solver.py:459-476).
//   r1          r1_reg: 0.5 * mean_b sum_{h,w,c<3} g^2 over the NHWC-4 image gradient g [B][H][W][4] (lane 3 is
//               padding: read, never used) and its backward u = gout * g / B (lane 3 written 0).
//   bce_logits  adv_loss fused with the domain gather: mean_b softplus(-+z[b][y[b]]) over the head's output
//               z [B][D] (D = the padded domain count) and device-resident domain ids y [B]; the backward writes the
//               dense [B][D] gradient, zero off the selected column.
// Both forwards accumulate in fp64 in a fixed order (a grid that depends on the size alone, wave shuffles, one
// finishing block): no float atomics, two runs are bit-equal.  The backwards read the upstream scalar gradient from
// device memory (no host sync).
#include "common.h"

namespace vst {

__device__ __forceinline__ double block_sum_d(double v, double* red) {
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

__global__ void r1_part_k(const float4* __restrict__ g, double* __restrict__ part, long npix) {
  __shared__ double red[4];
  double acc = 0.0;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
    const float4 v = g[p];
    acc += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z;
  }
  const double s = block_sum_d(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ void r1_finish_k(const double* __restrict__ part, int n, float* __restrict__ out, double scale) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) acc += part[i];
  const double s = block_sum_d(acc, red);
  if (threadIdx.x == 0) out[0] = (float)(s * scale);
}

__global__ void r1_bwd_k(const float4* __restrict__ g, const float* __restrict__ gout, float4* __restrict__ u,
                         long npix, float batch) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= npix) return;
  const float k = gout[0] / batch;
  const float4 v = g[p];
  u[p] = make_float4(k * v.x, k * v.y, k * v.z, 0.f);
}

__device__ __forceinline__ float sigmoid_f(float v) {
  if (v >= 0.f) return 1.f / (1.f + expf(-v));
  const float e = expf(v);
  return e / (1.f + e);
}

__global__ void bce_logits_fwd_k(const float* __restrict__ z, const long* __restrict__ y, float* __restrict__ loss,
                                 int B, int D, int nd, int target) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int b = threadIdx.x; b < B; b += 256) {
    const long c = y[b];
    if (c < 0 || c >= nd) {  // a domain id outside the head: no read, the loss says so
      acc += (double)NAN;
      continue;
    }
    const double v = (double)z[(long)b * D + c];
    acc += fmax(v, 0.0) - (target ? v : 0.0) + log1p(exp(-fabs(v)));
  }
  const double s = block_sum_d(acc, red);
  if (threadIdx.x == 0) loss[0] = (float)(s / (double)B);
}

__global__ void bce_logits_bwd_k(const float* __restrict__ z, const long* __restrict__ y,
                                 const float* __restrict__ gout, float* __restrict__ grad, int B, int D, int nd,
                                 int target) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * D) return;
  const int b = (int)(i / D), c = (int)(i % D);
  const long s = y[b];
  float g = 0.f;
  if (s < 0 || s >= nd) {
    g = NAN;
  } else if (c == s) {
    const float v = z[i];
    // sigmoid(v) - target without the cancellation at large |v|: sigmoid(v) - 1 = -sigmoid(-v)
    g = (target ? -sigmoid_f(-v) : sigmoid_f(v)) / (float)B * gout[0];
  }
  grad[i] = g;
}

static int r1_blocks(long npix) {
  const long nb = (npix + 255) / 256;
  return (int)(nb < VST_R1_PART_DOUBLES ? nb : VST_R1_PART_DOUBLES);
}

static bool bce_args(const void* z, const void* y, const void* a, const void* b, int B, int D, int nd,
                     float target) {
  return z && y && a && b && B > 0 && D > 0 && D % 4 == 0 && nd > 0 && nd <= D && (target == 0.f || target == 1.f);
}

}  // namespace vst

using namespace vst;

extern "C" int vst_loss_r1(const float* g, float* loss, double* part, int B, long hw, void* stream) {
  VST_REQUIRE(g && loss && part && B > 0 && hw > 0, "loss_r1: bad args");
  hipStream_t s = (hipStream_t)stream;
  const long npix = (long)B * hw;
  const int nb = r1_blocks(npix);
  hipLaunchKernelGGL(r1_part_k, dim3(nb), dim3(256), 0, s, (const float4*)g, part, npix);
  hipLaunchKernelGGL(r1_finish_k, dim3(1), dim3(256), 0, s, part, nb, loss, 0.5 / (double)B);
  return check_launch("loss_r1");
}

extern "C" int vst_loss_r1_bwd(const float* g, const float* gout, float* u, int B, long hw, void* stream) {
  VST_REQUIRE(g && gout && u && B > 0 && hw > 0, "loss_r1_bwd: bad args");
  const long npix = (long)B * hw;
  VST_REQUIRE((npix + 255) / 256 <= 0x7fffffffL, "loss_r1_bwd: too many pixels for one grid");
  hipLaunchKernelGGL(r1_bwd_k, dim3(ceil_div(npix, 256)), dim3(256), 0, (hipStream_t)stream, (const float4*)g, gout,
                     (float4*)u, npix, (float)B);
  return check_launch("loss_r1_bwd");
}

extern "C" int vst_loss_bce_logits(const float* z, const long* y, float* loss, int B, int D, int nd, float target,
                                   void* stream) {
  VST_REQUIRE(bce_args(z, y, loss, loss, B, D, nd, target),
              "loss_bce_logits: bad args (D %% 4 == 0, 0 < nd <= D, target 0 or 1)");
  hipLaunchKernelGGL(bce_logits_fwd_k, dim3(1), dim3(256), 0, (hipStream_t)stream, z, y, loss, B, D, nd,
                     target == 1.f ? 1 : 0);
  return check_launch("loss_bce_logits");
}

extern "C" int vst_loss_bce_logits_bwd(const float* z, const long* y, const float* gout, float* grad, int B, int D,
                                       int nd, float target, void* stream) {
  VST_REQUIRE(bce_args(z, y, gout, grad, B, D, nd, target),
              "loss_bce_logits_bwd: bad args (D %% 4 == 0, 0 < nd <= D, target 0 or 1)");
  hipLaunchKernelGGL(bce_logits_bwd_k, dim3(ceil_div((long)B * D, 256)), dim3(256), 0, (hipStream_t)stream, z, y,
                     gout, grad, B, D, nd, target == 1.f ? 1 : 0);
  return check_launch("loss_bce_logits_bwd");
}
