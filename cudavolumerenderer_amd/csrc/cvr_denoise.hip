// cvr_denoise.hip - the variance-guided a-trous denoiser on the per-pixel moments
// (cvr_denoise*, include/cvr.h).  The arithmetic is denoise_prepare / denoise_pass /
// denoise_final of cvr_kernels.h, the definitions cvr_denoise_host runs on the CPU: these
// kernels only map pixels onto lanes, so device and host agree bit for bit.
//
// One lane per pixel, 256-thread workgroups over tiles of 32 x 8 pixels (a wave covers two
// 32-pixel rows: its centre loads are two 512-byte runs).  The 25 taps of a pass of step 4 and
// above are plain global loads: the image is read 25 times from L1 / L2 and once from HBM or
// the Infinity Cache (16 B per pixel; 1024^2 is 16 MiB per image); steps 1 and 2 read their
// taps from an LDS copy of the tile and its halo.  Lanes of a partial tile are masked and never
// leave before the one barrier; no atomics, no waits on other waves, every loop bounded.
#include "cvr_kernels.h"

// 1 (default): the passes of step 1 and 2 stage their tile in LDS (measured faster with the same
// bits, profiles/denoise/README.md); 0 (`make variant-dnplain`): every pass takes global loads.
#ifndef CVR_DENOISE_LDS
#define CVR_DENOISE_LDS 1
#endif

namespace cvr {
namespace {

constexpr uint32_t kTileW = 32, kTileH = 8;

// The pixel of this lane, and whether it lies in the image: tiles row-major over a 1-D grid.
__device__ __forceinline__ bool denoise_pixel(uint32_t w, uint32_t h, uint32_t& x, uint32_t& y) {
  const uint32_t tiles_x = (w + kTileW - 1u) / kTileW;
  const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  x = tx * kTileW + (threadIdx.x & (kTileW - 1u));
  y = ty * kTileH + (threadIdx.x >> 5);
  return x < w && y < h;
}

__global__ __launch_bounds__(256) void k_denoise_prepare(const float4* __restrict__ sum, const float4* __restrict__ m2,
                                                         uint32_t w, uint32_t h, uint32_t n_samples,
                                                         const uint32_t* __restrict__ counts, float4* __restrict__ img) {
  uint32_t x, y;
  if (denoise_pixel(w, h, x, y)) {
    const size_t i = (size_t)y * w + x;
    img[i] = denoise_prepare(sum[i], m2[i], denoise_count(counts, n_samples, w, x, y));
  }
}

// kLast: the pass that ends the filter stores the output image instead of the next pass's input.
// The guided filter's passes (cvr_denoise_guided*): instances of their own below, the unguided
// kernels' text and instruction streams stay as they were.
template <bool kLast, class Guide>
__device__ __forceinline__ void denoise_pass_body(const float4* __restrict__ src, float4* __restrict__ dst, uint32_t w,
                                                  uint32_t h, uint32_t step, float sigma, float floor,
                                                  const float4* __restrict__ sum, uint32_t n_samples,
                                                  const uint32_t* __restrict__ counts, float* __restrict__ out_var,
                                                  const Guide& guide) {
  uint32_t x, y;
  if (denoise_pixel(w, h, x, y)) {
    const size_t i = (size_t)y * w + x;
    const float4 f = denoise_pass(src, w, h, x, y, step, sigma, floor, guide);
    if (kLast) {
      dst[i] = denoise_final(f, sum[i], denoise_count(counts, n_samples, w, x, y));
      if (out_var) out_var[i] = f.w < 0.0f ? -1.0f : f.w;
    } else {
      dst[i] = f;
    }
  }
}
template <bool kLast>
__global__ __launch_bounds__(256) void k_denoise_pass(const float4* __restrict__ src, float4* __restrict__ dst,
                                                      uint32_t w, uint32_t h, uint32_t step, float sigma, float floor,
                                                      const float4* __restrict__ sum, uint32_t n_samples,
                                                      const uint32_t* __restrict__ counts, float* __restrict__ out_var) {
  uint32_t x, y;
  if (denoise_pixel(w, h, x, y)) {
    const size_t i = (size_t)y * w + x;
    const float4 f = denoise_pass(src, w, h, x, y, step, sigma, floor);
    if (kLast) {
      dst[i] = denoise_final(f, sum[i], denoise_count(counts, n_samples, w, x, y));
      if (out_var) out_var[i] = f.w < 0.0f ? -1.0f : f.w;
    } else {
      dst[i] = f;
    }
  }
}
template <bool kLast>
__global__ __launch_bounds__(256) void k_denoise_pass_guided(const float4* __restrict__ src, float4* __restrict__ dst,
                                                             uint32_t w, uint32_t h, uint32_t step, float sigma,
                                                             float floor, const float4* __restrict__ sum,
                                                             uint32_t n_samples, const uint32_t* __restrict__ counts,
                                                             float* __restrict__ out_var, const DenoiseGuide guide) {
  denoise_pass_body<kLast>(src, dst, w, h, step, sigma, floor, sum, n_samples, counts, out_var, guide);
}

#if CVR_DENOISE_LDS
// The passes with step S = 1 and 2 stage their tile plus a halo of 2 S pixels in LDS first
// (36 x 12 or 40 x 16 float4), so every pixel is loaded from global memory once per workgroup
// and the 34 taps read LDS: 8 % / 17 % faster per pass at 1024^2 / 4096^2 than global taps
// (profiles/denoise/README.md).  The same denoise_pass_at in the same order: the same bits.
// Every lane reaches the barrier (a lane outside the image stages, then stores nothing).
template <uint32_t S>
struct DenoiseLdsTile {
  static constexpr int R = 2 * (int)S, LW = (int)kTileW + 2 * R, LH = (int)kTileH + 2 * R;
  const float4* tile;
  int x0, y0;  // image coordinate of tile[0]
  __device__ float4 operator()(int qx, int qy) const { return tile[(qy - y0) * LW + (qx - x0)]; }
};
template <bool kLast, uint32_t S, class Guide>
__device__ __forceinline__ void denoise_pass_lds_body(float4* tile, const float4* __restrict__ src,
                                                      float4* __restrict__ dst, uint32_t w, uint32_t h, float sigma,
                                                      float floor, const float4* __restrict__ sum, uint32_t n_samples,
                                                      const uint32_t* __restrict__ counts, float* __restrict__ out_var,
                                                      const Guide& guide) {
  using T = DenoiseLdsTile<S>;
  uint32_t x, y;
  const bool inside = denoise_pixel(w, h, x, y);
  const int x0 = (int)(x - (threadIdx.x & (kTileW - 1u))) - T::R, y0 = (int)(y - (threadIdx.x >> 5)) - T::R;
  for (int i = (int)threadIdx.x; i < T::LW * T::LH; i += 256) {
    const int ly = i / T::LW, lx = i - ly * T::LW, gx = x0 + lx, gy = y0 + ly;
    // (a position outside the image is never asked for: any value does)
    tile[i] = (gx >= 0 && gx < (int)w && gy >= 0 && gy < (int)h) ? src[(size_t)gy * w + (size_t)gx]
                                                                 : make_float4(0.0f, 0.0f, 0.0f, -1.0f);
  }
  __syncthreads();
  if (inside) {
    const size_t i = (size_t)y * w + x;
    const float4 f = denoise_pass_at(T{tile, x0, y0}, w, h, x, y, S, sigma, floor, guide);
    if (kLast) {
      dst[i] = denoise_final(f, sum[i], denoise_count(counts, n_samples, w, x, y));
      if (out_var) out_var[i] = f.w < 0.0f ? -1.0f : f.w;
    } else {
      dst[i] = f;
    }
  }
}
template <bool kLast, uint32_t S>
__global__ __launch_bounds__(256) void k_denoise_pass_lds(const float4* __restrict__ src, float4* __restrict__ dst,
                                                          uint32_t w, uint32_t h, float sigma, float floor,
                                                          const float4* __restrict__ sum, uint32_t n_samples,
                                                          const uint32_t* __restrict__ counts,
                                                          float* __restrict__ out_var) {
  using T = DenoiseLdsTile<S>;
  __shared__ float4 tile[T::LW * T::LH];
  uint32_t x, y;
  const bool inside = denoise_pixel(w, h, x, y);
  const int x0 = (int)(x - (threadIdx.x & (kTileW - 1u))) - T::R, y0 = (int)(y - (threadIdx.x >> 5)) - T::R;
  for (int i = (int)threadIdx.x; i < T::LW * T::LH; i += 256) {
    const int ly = i / T::LW, lx = i - ly * T::LW, gx = x0 + lx, gy = y0 + ly;
    // (a position outside the image is never asked for: any value does)
    tile[i] = (gx >= 0 && gx < (int)w && gy >= 0 && gy < (int)h) ? src[(size_t)gy * w + (size_t)gx]
                                                                 : make_float4(0.0f, 0.0f, 0.0f, -1.0f);
  }
  __syncthreads();
  if (inside) {
    const size_t i = (size_t)y * w + x;
    const float4 f = denoise_pass_at(T{tile, x0, y0}, w, h, x, y, S, sigma, floor);
    if (kLast) {
      dst[i] = denoise_final(f, sum[i], denoise_count(counts, n_samples, w, x, y));
      if (out_var) out_var[i] = f.w < 0.0f ? -1.0f : f.w;
    } else {
      dst[i] = f;
    }
  }
}
// (the feature planes are read from global memory: two pixels per tap, never filtered)
template <bool kLast, uint32_t S>
__global__ __launch_bounds__(256) void k_denoise_pass_lds_guided(const float4* __restrict__ src,
                                                                 float4* __restrict__ dst, uint32_t w, uint32_t h,
                                                                 float sigma, float floor, const float4* __restrict__ sum,
                                                                 uint32_t n_samples, const uint32_t* __restrict__ counts,
                                                                 float* __restrict__ out_var, const DenoiseGuide guide) {
  __shared__ float4 tile[DenoiseLdsTile<S>::LW * DenoiseLdsTile<S>::LH];
  denoise_pass_lds_body<kLast, S>(tile, src, dst, w, h, sigma, floor, sum, n_samples, counts, out_var, guide);
}
#endif

uint32_t denoise_grid(uint32_t w, uint32_t h) {
  return ((w + kTileW - 1u) / kTileW) * ((h + kTileH - 1u) / kTileH);
}
// (the callers in cvr_api.cpp check these too: an image of at most 2^24 pixels, a count map
// only over sides that are multiples of 8)
bool denoise_shape_ok(uint32_t w, uint32_t h, const uint32_t* counts) {
  return w && h && (uint64_t)w * h <= (1ull << 24) && !(counts && (w % 8u || h % 8u));
}

}  // namespace

hipError_t launch_denoise_prepare(const float4* sum, const float4* m2, uint32_t w, uint32_t h, uint32_t n_samples,
                                  const uint32_t* counts, float4* img, hipStream_t s) {
  if (!denoise_shape_ok(w, h, counts) || !sum || !m2 || !img) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_denoise_prepare, dim3(denoise_grid(w, h)), dim3(256), 0, s, sum, m2, w, h, n_samples, counts, img);
  return hipGetLastError();
}

// One pass on stream s: the LDS-staged kernel for steps 1 and 2, plain taps above; guided instances with a guide.
template <bool kLast>
static void denoise_pass_dispatch(const float4* src, float4* dst, uint32_t w, uint32_t h, uint32_t step, float sigma,
                                  float floor, const float4* sum, uint32_t n_samples, const uint32_t* counts,
                                  float* out_var, const DenoiseGuide* guide, hipStream_t s) {
  const dim3 grid(denoise_grid(w, h)), block(256);
#if CVR_DENOISE_LDS
  if (step <= 2u) {
    if (guide) {
      if (step == 1u)
        hipLaunchKernelGGL((k_denoise_pass_lds_guided<kLast, 1>), grid, block, 0, s, src, dst, w, h, sigma, floor, sum,
                           n_samples, counts, out_var, *guide);
      else
        hipLaunchKernelGGL((k_denoise_pass_lds_guided<kLast, 2>), grid, block, 0, s, src, dst, w, h, sigma, floor, sum,
                           n_samples, counts, out_var, *guide);
    } else {
      if (step == 1u)
        hipLaunchKernelGGL((k_denoise_pass_lds<kLast, 1>), grid, block, 0, s, src, dst, w, h, sigma, floor, sum,
                           n_samples, counts, out_var);
      else
        hipLaunchKernelGGL((k_denoise_pass_lds<kLast, 2>), grid, block, 0, s, src, dst, w, h, sigma, floor, sum,
                           n_samples, counts, out_var);
    }
    return;
  }
#endif
  if (guide)
    hipLaunchKernelGGL(k_denoise_pass_guided<kLast>, grid, block, 0, s, src, dst, w, h, step, sigma, floor, sum,
                       n_samples, counts, out_var, *guide);
  else
    hipLaunchKernelGGL(k_denoise_pass<kLast>, grid, block, 0, s, src, dst, w, h, step, sigma, floor, sum, n_samples,
                       counts, out_var);
}
static bool denoise_guide_ok(const DenoiseGuide* g) {
  return !g || (g->rgba && g->depth && !((uintptr_t)g->rgba & 15u) && !((uintptr_t)g->depth & 3u));
}

hipError_t launch_denoise_pass(const float4* src, float4* dst, uint32_t w, uint32_t h, uint32_t step, float sigma,
                               float floor, hipStream_t s, const DenoiseGuide* guide) {
  if (!denoise_shape_ok(w, h, nullptr) || !src || !dst || src == dst || step == 0 || step > 32u || !denoise_guide_ok(guide))
    return hipErrorInvalidValue;
  denoise_pass_dispatch<false>(src, dst, w, h, step, sigma, floor, nullptr, 0u, nullptr, nullptr, guide, s);
  return hipGetLastError();
}

hipError_t launch_denoise_last(const float4* src, uint32_t w, uint32_t h, uint32_t step, float sigma, float floor,
                               const float4* sum, uint32_t n_samples, const uint32_t* counts, float4* out_rgba,
                               float* out_var, hipStream_t s, const DenoiseGuide* guide) {
  if (!denoise_shape_ok(w, h, counts) || !src || !sum || !out_rgba || src == out_rgba || step == 0 || step > 32u ||
      !denoise_guide_ok(guide))
    return hipErrorInvalidValue;
  denoise_pass_dispatch<true>(src, out_rgba, w, h, step, sigma, floor, sum, n_samples, counts, out_var, guide, s);
  return hipGetLastError();
}

}  // namespace cvr
