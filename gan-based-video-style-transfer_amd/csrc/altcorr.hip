// RAFT's memory-saving correlation (utils/raft/raft/corr.py:63-91 AlternateCorrBlock): the window
// lookup computed from the two feature maps, without the all-pairs volume.
//
// avg_pool2d and bilinear sampling are linear, so pooling the volume over (h2, w2) equals correlating
// with a pooled fmap2, and interpolating correlations equals interpolating dot products:
//   fmap2 pyramid   levels 1..L-1 = 2x2 average pools (floor) of NHWC fmap2, packed in one buffer
//   window lookup   per (pixel, level): the (2r+2)^2 dot products of fmap1[b,h,w,:] with the level's patch
//                   at floor(coords / 2^lvl) + (-r .. r+1), blended into the (2r+1)^2 outputs (all of
//                   them share one fractional offset), the blend divided by sqrt(D)
// fp32 FMA throughout, no atomics (two runs agree bit for bit), independent of the conv math mode.
#include "common.h"

namespace vst {

// Level l (0-based) of the pyramid: off[l] floats into the pooled buffer (level 0 is fmap2 itself,
// off[0] unused), h[l] x w[l] positions of Dp channels per image.
struct AltGeom {
  long off[8];
  int h[8], w[8];
};

// y[b][ho][wo][:] = avg of the 2x2 block of x (floor mode: an odd last row / column is dropped);
// ATen's summation order ((x00 + x01) + x10) + x11, then / 4.  One thread per float4.
__global__ void altcorr_pool_k(const float* __restrict__ x, float* __restrict__ y, int B, int H, int W,
                               int Dp) {
  const int Ho = H / 2, Wo = W / 2, D4 = Dp / 4;
  const long total = (long)B * Ho * Wo * D4;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int d = (int)(i % D4);
  const long p = i / D4;
  const int wo = (int)(p % Wo), ho = (int)((p / Wo) % Ho);
  const long b = p / ((long)Wo * Ho);
  const float4* s = reinterpret_cast<const float4*>(x) + ((b * H + 2 * ho) * W + 2 * wo) * D4 + d;
  float4 a = s[0];
  add_f4(a, s[D4]);
  add_f4(a, s[(long)W * D4]);
  add_f4(a, s[(long)W * D4 + D4]);
  a.x *= 0.25f; a.y *= 0.25f; a.z *= 0.25f; a.w *= 0.25f;
  reinterpret_cast<float4*>(y)[i] = a;
}

#define ALT_WAVES 4       // waves (work items) per block
#define ALT_MAXK2 16      // 2 * radius + 2 <= 16 (radius <= 7)
#define ALT_LPP 8         // lanes per patch position: a wave instruction covers 64 / ALT_LPP = 8 positions
#define ALT_REG_CHUNKS 8  // fmap1 of up to 8 x 32 channels is held in registers

// One wave per (pixel, level).  8 lanes share one patch position: each reads a contiguous 32-channel
// (128-byte) chunk of the position's channel vector as float4, so a wave instruction covers 8 positions;
// the 8 partial sums are folded with 3 xor-shuffles.  The (2r+2)^2 dots (zero outside the level) go through
// LDS to the blend, one lane per output, which divides by sqrt(D).  REG: Dp <= 256, fmap1 stays in registers.
template <bool REG>
__global__ __launch_bounds__(64 * ALT_WAVES) void altcorr_lookup_k(
    const float* __restrict__ f1, const float* __restrict__ f2, const float* __restrict__ pyr, const AltGeom geo,
    const float* __restrict__ coords, float* __restrict__ out, int B, int H, int W, int Dp, int D, int levels,
    int r, int Cs, long items, int tiles) {
  __shared__ float dots[ALT_WAVES][ALT_MAXK2 * ALT_MAXK2];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: what follows is scalar
  const int lane = threadIdx.x & 63, grp = lane / ALT_LPP, sub = lane % ALT_LPP;
  const long item0 = (long)xcd_tile(blockIdx.x, tiles) * ALT_WAVES + wave;
  const bool live = item0 < items;  // a wave past the end works on the last item and writes nothing
  const long item = live ? item0 : items - 1;
  const int lvl = (int)(item % levels);
  const long pix = item / levels;
  const int w = (int)(pix % W), h = (int)((pix / W) % H);
  const long b = pix / ((long)W * H);
  const int K = 2 * r + 1, K2 = K + 1, KK = K * K, npos = K2 * K2;
  const int Hl = geo.h[lvl], Wl = geo.w[lvl];
  const float inv = 1.f / (float)(1 << lvl);  // a power of two: the same value as coords / 2^lvl
  const float px = coords[((b * 2) * H + h) * W + w] * inv;
  const float py = coords[((b * 2 + 1) * H + h) * W + w] * inv;
  // far outside either way: clamped so that the integer arithmetic below cannot overflow
  const float fx0 = fminf(fmaxf(floorf(px), -16777216.f), 16777216.f);
  const float fy0 = fminf(fmaxf(floorf(py), -16777216.f), 16777216.f);
  const int x0 = (int)fx0 - r, y0 = (int)fy0 - r;  // the patch's first column / row
  const float we = px - fx0, wn = py - fy0;
  const float* lv = (lvl == 0 ? f2 : pyr + geo.off[lvl]) + b * Hl * Wl * Dp;
  const float* a1 = f1 + pix * Dp;
  const int nch = (Dp + 4 * ALT_LPP - 1) / (4 * ALT_LPP);
  float4 a[ALT_REG_CHUNKS];
  if (REG) {
#pragma unroll
    for (int c = 0; c < ALT_REG_CHUNKS; ++c) {
      const int d = (c * ALT_LPP + sub) * 4;
      a[c] = d < Dp ? *reinterpret_cast<const float4*>(a1 + d) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  int j = grp / K2, i = grp % K2;  // this lane group's position (row j, column i), advanced by 8 per round
  for (int p0 = 0; p0 < npos; p0 += 64 / ALT_LPP) {
    const int p = p0 + grp;  // p >= npos: an idle group
    const int yy = y0 + j, xx = x0 + i;
    const bool in = p < npos && (unsigned)yy < (unsigned)Hl && (unsigned)xx < (unsigned)Wl;
    // load from a clamped (always valid) address, zero by select
    const int yc = min(max(yy, 0), Hl - 1), xc = min(max(xx, 0), Wl - 1);
    const float* q = lv + ((long)yc * Wl + xc) * Dp;
    float s = 0.f;
    if (REG) {
      // no branch around the loads, so that all of them are in flight together: a chunk past Dp reads
      // channels 0..3 instead and meets a[c] == 0
      float4 v[ALT_REG_CHUNKS];
#pragma unroll
      for (int c = 0; c < ALT_REG_CHUNKS; ++c) {
        const int d = (c * ALT_LPP + sub) * 4;
        v[c] = *reinterpret_cast<const float4*>(q + (d < Dp ? d : 0));
      }
#pragma unroll
      for (int c = 0; c < ALT_REG_CHUNKS; ++c) {
        s = fmaf(a[c].x, v[c].x, s);
        s = fmaf(a[c].y, v[c].y, s);
        s = fmaf(a[c].z, v[c].z, s);
        s = fmaf(a[c].w, v[c].w, s);
      }
    } else {
      for (int c = 0; c < nch; ++c) {
        const int d = (c * ALT_LPP + sub) * 4;
        if (d < Dp) {
          const float4 u = *reinterpret_cast<const float4*>(a1 + d);
          const float4 v = *reinterpret_cast<const float4*>(q + d);
          s = fmaf(u.x, v.x, s);
          s = fmaf(u.y, v.y, s);
          s = fmaf(u.z, v.z, s);
          s = fmaf(u.w, v.w, s);
        }
      }
    }
#pragma unroll
    for (int o = ALT_LPP / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (sub == 0 && p < npos) dots[wave][p] = in ? s : 0.f;
    i += 64 / ALT_LPP;
    while (i >= K2) {  // K2 >= 2: at most 4 turns
      i -= K2;
      ++j;
    }
  }
  __syncthreads();
  if (!live) return;
  const float e = 1.f - we, s_ = 1.f - wn, sq = sqrtf((float)D);
  float* o = out + pix * Cs;
  for (int t = lane; t < KK; t += 64) {
    const int ai = t / K, ci = t % K;  // channel a*(2r+1) + c: x offset a - r, y offset c - r
    const float* dd = &dots[wave][ci * K2 + ai];
    o[lvl * KK + t] = (dd[0] * (s_ * e) + dd[1] * (s_ * we) + dd[K2] * (wn * e) + dd[K2 + 1] * (wn * we)) / sq;
  }
  if (lvl == 0)
    for (int t = levels * KK + lane; t < Cs; t += 64) o[t] = 0.f;
}

}  // namespace vst

using namespace vst;

// Fills the level geometry; returns the pooled buffer's floats, or -1 for levels outside 1..8.
static long alt_geom(long B, int H, int W, int Dp, int levels, AltGeom* g) {
  if (levels < 1 || levels > 8) return -1;
  long o = 0;
  int h = H, w = W;
  for (int l = 0; l < 8; ++l) {
    g->off[l] = 0;
    g->h[l] = g->w[l] = 0;
  }
  g->h[0] = H;
  g->w[0] = W;
  for (int l = 1; l < levels; ++l) {
    h /= 2;
    w /= 2;
    g->off[l] = o;
    g->h[l] = h;
    g->w[l] = w;
    o += B * (long)h * w * Dp;
  }
  return o;
}

extern "C" long vst_altcorr_pyramid_floats(int B, int H, int W, int Dp, int levels) {
  AltGeom g;
  return alt_geom(B, H, W, Dp, levels, &g);
}

extern "C" int vst_altcorr_pyramid(const float* f2, float* pyr, int B, int H, int W, int Dp, int levels,
                                   void* stream) {
  VST_REQUIRE(f2 && (pyr || levels == 1) && B > 0 && H > 0 && W > 0 && Dp > 0 && Dp % 4 == 0 && levels >= 1 &&
                  levels <= 8,
              "altcorr_pyramid: bad args");
  AltGeom g;
  alt_geom(B, H, W, Dp, levels, &g);
  for (int l = 0; l < levels; ++l)
    VST_REQUIRE(g.h[l] >= 2 && g.w[l] >= 2, "altcorr_pyramid: level %d smaller than 2x2", l);
  for (int l = 1; l < levels; ++l) {
    const long total = (long)B * g.h[l] * g.w[l] * (Dp / 4);
    VST_REQUIRE(total <= 0x7fffffffL * 256, "altcorr_pyramid: level %d too large for one launch", l);
    hipLaunchKernelGGL(altcorr_pool_k, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       l == 1 ? f2 : pyr + g.off[l - 1], pyr + g.off[l], B, g.h[l - 1], g.w[l - 1], Dp);
  }
  return check_launch("altcorr_pyramid");
}

extern "C" int vst_altcorr_lookup(const float* f1, const float* f2, const float* pyr, const float* coords,
                                  float* out, int B, int H, int W, int Dp, int D, int levels, int radius, int Cs,
                                  void* stream) {
  VST_REQUIRE(f1 && f2 && (pyr || levels == 1) && coords && out && B > 0 && H > 0 && W > 0 && Dp > 0 &&
                  Dp % 4 == 0 && D > 0 && D <= Dp && levels >= 1 && levels <= 8 && radius >= 0 &&
                  2 * radius + 2 <= ALT_MAXK2 && Cs >= levels * (2 * radius + 1) * (2 * radius + 1),
              "altcorr_lookup: bad args");
  AltGeom g;
  alt_geom(B, H, W, Dp, levels, &g);
  for (int l = 0; l < levels; ++l)
    VST_REQUIRE(g.h[l] >= 2 && g.w[l] >= 2, "altcorr_lookup: level %d smaller than 2x2", l);
  const long items = (long)B * H * W * levels;
  const long tiles = (items + ALT_WAVES - 1) / ALT_WAVES;
  VST_REQUIRE(tiles <= 0x7fffffffL, "altcorr_lookup: too many pixels for one launch");
  // the level geometry travels as a by-value kernel argument (graph-capturable, no host sync)
  if (Dp <= 4 * ALT_LPP * ALT_REG_CHUNKS)
    hipLaunchKernelGGL(altcorr_lookup_k<true>, dim3((unsigned)tiles), dim3(64 * ALT_WAVES), 0, (hipStream_t)stream,
                       f1, f2, pyr, g, coords, out, B, H, W, Dp, D, levels, radius, Cs, items, (int)tiles);
  else
    hipLaunchKernelGGL(altcorr_lookup_k<false>, dim3((unsigned)tiles), dim3(64 * ALT_WAVES), 0, (hipStream_t)stream,
                       f1, f2, pyr, g, coords, out, B, H, W, Dp, D, levels, radius, Cs, items, (int)tiles);
  return check_launch("altcorr_lookup");
}
