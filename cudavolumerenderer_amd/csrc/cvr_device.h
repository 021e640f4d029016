// cvr_device.h - device-only pieces that the medium build's and the field's kernels share: the
// wave reductions.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cvr {

// Every lane of the wave calls these and gets the wave's result.
template <class T>
__device__ __forceinline__ T wave_max(T v) {
  for (int o = 32; o; o >>= 1) {
    const T t = __shfl_xor(v, o);
    v = t > v ? t : v;
  }
  return v;
}
template <class T>
__device__ __forceinline__ T wave_min(T v) {
  for (int o = 32; o; o >>= 1) {
    const T t = __shfl_xor(v, o);
    v = t < v ? t : v;
  }
  return v;
}
__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
  for (int o = 32; o; o >>= 1) v |= __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

}  // namespace cvr
