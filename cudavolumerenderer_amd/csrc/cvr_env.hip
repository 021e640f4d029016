// cvr_env.hip - environment maps (cvr_set_environment, cvr_environment_eval): the conversion of a
// caller's 3- or 4-channel image in device memory to the stored float4 texels, with the scan of what
// was stored, and the lookup for arbitrary directions (the parity hook that is independent of the walk).
#include <hip/hip_runtime.h>

#include "cvr_env.h"

namespace cvr {

namespace {

// dst[i] = (fl(scale r), fl(scale g), fl(scale b), 0) of texel i, in one pass that also reduces the
// largest stored component and the smallest index of one that is negative or not finite.  Every
// thread takes texels tid, tid + threads, ...: a wave's loads and stores are contiguous.
__global__ __launch_bounds__(256) void k_env_convert(const float* __restrict__ src, uint32_t channels, size_t n,
                                                     float scale, float4* __restrict__ dst, EnvScan* __restrict__ scan) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  uint32_t mx = 0u;
  unsigned long long bad = ~0ull;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float c[3];
    if (channels == 4u) {
      const float4 t = reinterpret_cast<const float4*>(src)[i];
      c[0] = t.x;
      c[1] = t.y;
      c[2] = t.z;
    } else {
      c[0] = src[3 * i];
      c[1] = src[3 * i + 1];
      c[2] = src[3 * i + 2];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      c[k] = scale * c[k];
      // (>= +0 and finite: the bits of such floats order as unsigned integers)
      if (c[k] >= 0.0f && c[k] - c[k] == 0.0f) {
        const uint32_t b = __float_as_uint(c[k]) & 0x7FFFFFFFu;
        mx = b > mx ? b : mx;
      } else {
        const unsigned long long at = (unsigned long long)i * channels + (unsigned)k;
        bad = at < bad ? at : bad;
      }
    }
    dst[i] = make_float4(c[0], c[1], c[2], 0.0f);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t om = (uint32_t)__shfl_xor((int)mx, off);
    const unsigned long long ob = __shfl_xor(bad, off);
    mx = om > mx ? om : mx;
    bad = ob < bad ? ob : bad;
  }
  if ((threadIdx.x & 63u) == 0u) {
    if (mx != 0u) atomicMax(&scan->max_bits, mx);
    if (bad != ~0ull) atomicMin(&scan->first_bad, bad);
  }
}

__global__ __launch_bounds__(256) void k_env_eval(const EnvParams* __restrict__ Ep, const float* __restrict__ dirs,
                                                  size_t n, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const EnvParams E = *Ep;
  float rgb[3];
  env_lookup(E, dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], rgb);
  out[3 * i] = rgb[0];
  out[3 * i + 1] = rgb[1];
  out[3 * i + 2] = rgb[2];
}

}  // namespace

hipError_t launch_env_convert(const float* src, uint32_t channels, size_t n_texels, float scale, float4* dst,
                              EnvScan* scan, hipStream_t s) {
  if (n_texels == 0) return hipSuccess;
  const size_t blocks = (n_texels + 255) / 256;
  const uint32_t grid = (uint32_t)(blocks < 4096 ? blocks : 4096);
  hipLaunchKernelGGL(k_env_convert, dim3(grid), dim3(256), 0, s, src, channels, n_texels, scale, dst, scan);
  return hipGetLastError();
}

hipError_t launch_env_eval(const EnvParams* E, const float* dirs, size_t n, float* out, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_env_eval, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, E, dirs, n, out);
  return hipGetLastError();
}

}  // namespace cvr
