// cvr_medium_build.hip - the device-side front end of cvr_set_medium_device (gfx950): what the
// host uploads decide with loops over every voxel or leaf, decided here from the caller's device
// arrays.  Value scans (majorant, binary16 overflow, uniform albedo), the dense -> 8^3 leaves
// rule of cvr.h (leaf flags, exclusive scan, gather), the cell-leaf table and the empty-region
// mask.  The cells, bounds and brick words are then built by cvr_kernels.hip's kernels, unchanged.
//
// No kernel here waits on another workgroup: the exclusive scan is three launches (per-tile
// counts, one workgroup over the tile sums, scatter), ordered by the stream.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cvr_kernels.h"

namespace cvr {
namespace {

constexpr uint32_t kNoLeaf = 0xFFFFFFFFu;  // CVR_NO_LEAF
constexpr unsigned long long kNoIndex = ~0ull;
constexpr uint32_t kScanSteps = 8, kScanTile = 256 * kScanSteps;  // flags per workgroup of the scan

// finite and rounds to +-inf in binary16 (the host uploads' half_overflows)
__device__ __forceinline__ bool half_overflow(float f) {
  const float a = fabsf(f);
  return a >= 65520.0f && a < __builtin_huge_valf();
}
__device__ __forceinline__ uint32_t half_bits(float f) {
  const _Float16 h = (_Float16)f;
  return (uint32_t)__builtin_bit_cast(unsigned short, h);
}
__device__ __forceinline__ float wave_max(float v) {
  for (int o = 32; o; o >>= 1) {
    const float t = __shfl_xor(v, o);
    v = t > v ? t : v;
  }
  return v;
}
__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
  for (int o = 32; o; o >>= 1) {
    const unsigned long long t = __shfl_xor(v, o);
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

// ----------------------------------------------------------- value scans ---
// Streaming reads: consecutive lanes read consecutive 16 bytes (1 KiB per wave and load), a wave
// reduction, then at most one atomic of each kind per workgroup, and none when the result already
// holds what the workgroup found (the values only grow, fall or gain bits, so a stale read costs an
// atomic that changes nothing).  Atomics on one word are serialised at the memory side: with 8192
// workgroups each issuing theirs, C2's 60 MB density scan took 0.095 ms; with 2048 workgroups and
// the reads first, 0.026 ms (profiles/device_medium/README.md).
__global__ __launch_bounds__(256) void k_scan_density(const float* __restrict__ D, size_t n, uint32_t format,
                                                      MedScan* __restrict__ out) {
  float mx = 0.0f;  // max(0, every non-NaN voxel): a NaN or -0 never compares greater
  unsigned long long ov = kNoIndex;
  auto take = [&](float v, size_t i) {
    mx = v > mx ? v : mx;
    if (format && half_overflow(v) && i < ov) ov = i;
  };
  // 16 bytes per lane where the array's alignment allows it, the last n % 4 voxels one by one
  const size_t n4 = ((uintptr_t)D & 15u) ? 0 : n / 4;
  const float4* __restrict__ D4 = reinterpret_cast<const float4*>(D);
#pragma unroll 2
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const float4 v = D4[i];
    take(v.x, 4 * i);
    take(v.y, 4 * i + 1);
    take(v.z, 4 * i + 2);
    take(v.w, 4 * i + 3);
  }
  for (size_t i = 4 * n4 + (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) take(D[i], i);
  mx = wave_max(mx);
  ov = wave_min(ov);
  __shared__ float s_mx[4];
  __shared__ unsigned long long s_ov[4];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  if (lane == 0) {
    s_mx[w] = mx;
    s_ov[w] = ov;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t k = 1; k < 4; ++k) {
      mx = s_mx[k] > mx ? s_mx[k] : mx;
      ov = s_ov[k] < ov ? s_ov[k] : ov;
    }
    // mx >= +0, so its bits order as the values do
    if (__float_as_uint(mx) > __atomic_load_n(&out->max_bits, __ATOMIC_RELAXED))
      atomicMax(&out->max_bits, __float_as_uint(mx));
    if (ov < __atomic_load_n(&out->ovf_density, __ATOMIC_RELAXED)) atomicMin(&out->ovf_density, ov);
  }
}

// albedo_flags bit 0: some voxel's rgb differs from voxel 0's (format 1: the rounded halves; bits
// are compared, w is ignored); bit 1: some voxel's 16 bytes differ from voxel 0's (the leaf rule).
__global__ __launch_bounds__(256) void k_scan_albedo(const float4* __restrict__ A, size_t n, uint32_t format,
                                                     MedScan* __restrict__ out) {
  const float4 f = A[0];
  const uint32_t f0 = __float_as_uint(f.x), f1 = __float_as_uint(f.y), f2 = __float_as_uint(f.z),
                 f3 = __float_as_uint(f.w);
  const uint32_t h0 = half_bits(f.x), h1 = half_bits(f.y), h2 = half_bits(f.z);
  uint32_t flags = 0;
  unsigned long long ov = kNoIndex;
#pragma unroll 2
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float4 a = A[i];
    const bool rgb = __float_as_uint(a.x) != f0 || __float_as_uint(a.y) != f1 || __float_as_uint(a.z) != f2;
    if (rgb || __float_as_uint(a.w) != f3) flags |= 2u;
    if (format) {
      if (half_bits(a.x) != h0 || half_bits(a.y) != h1 || half_bits(a.z) != h2) flags |= 1u;
      const unsigned long long at =
          half_overflow(a.x) ? 4 * i : half_overflow(a.y) ? 4 * i + 1 : half_overflow(a.z) ? 4 * i + 2 : kNoIndex;
      ov = at < ov ? at : ov;
    } else if (rgb) {
      flags |= 1u;
    }
  }
  flags = wave_or(flags);
  ov = wave_min(ov);
  __shared__ uint32_t s_fl[4];
  __shared__ unsigned long long s_ov[4];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  if (lane == 0) {
    s_fl[w] = flags;
    s_ov[w] = ov;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t k = 1; k < 4; ++k) {
      flags |= s_fl[k];
      ov = s_ov[k] < ov ? s_ov[k] : ov;
    }
    if (flags & ~__atomic_load_n(&out->albedo_flags, __ATOMIC_RELAXED)) atomicOr(&out->albedo_flags, flags);
    if (ov < __atomic_load_n(&out->ovf_albedo, __ATOMIC_RELAXED)) atomicMin(&out->ovf_albedo, ov);
  }
}

// The context's albedo grid filled with one value (CVR_DEVMED_CONST_ALBEDO, dense).
__global__ __launch_bounds__(256) void k_fill_albedo(void* __restrict__ dst, size_t n, uint32_t format, float4 v) {
  uint2 h;
  h.x = half_bits(v.x) | half_bits(v.y) << 16;
  h.y = half_bits(v.z) | half_bits(v.w) << 16;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    if (format)
      reinterpret_cast<uint2*>(dst)[i] = h;
    else
      reinterpret_cast<float4*>(dst)[i] = v;
  }
}

// ------------------------------------------------------------- leaf flags ---
// flags[leaf] = 1 iff an in-grid voxel of the leaf has density != 0.0f (-0: no, NaN: yes) or 16
// albedo bytes other than voxel 0's.  One workgroup takes 32 leaves of one (lz, ly) row: its
// work-items are 256 consecutive x, so a wave reads 64-voxel x-runs of each of the row's 64
// (z, y) lines, not one leaf's 8-voxel rows; the 8 lanes of a leaf then OR their findings.
__global__ __launch_bounds__(256) void k_leaf_flags(const float* __restrict__ D, const float4* __restrict__ A,
                                                    uint32_t nx, uint32_t ny, uint32_t nz, uint32_t lnx, uint32_t lny,
                                                    uint32_t lnz, uint32_t* __restrict__ flags) {
  const uint32_t nxc = (lnx + 31u) / 32u;
  const size_t ntasks = (size_t)nxc * lny * lnz;
  uint32_t b0 = 0, b1 = 0, b2 = 0, b3 = 0;
  if (A) {
    const float4 f = A[0];
    b0 = __float_as_uint(f.x), b1 = __float_as_uint(f.y), b2 = __float_as_uint(f.z), b3 = __float_as_uint(f.w);
  }
  for (size_t t = blockIdx.x; t < ntasks; t += gridDim.x) {
    const uint32_t xc = (uint32_t)(t % nxc), ly = (uint32_t)((t / nxc) % lny), lz = (uint32_t)(t / ((size_t)nxc * lny));
    const uint32_t x = xc * 256u + threadIdx.x;
    uint32_t any = 0;
    if (x < nx) {
#pragma unroll 8
      for (uint32_t r = 0; r < 64u; ++r) {
        const uint32_t y = ly * 8u + (r & 7u), z = lz * 8u + (r >> 3);
        if (y < ny && z < nz) {
          const size_t i = ((size_t)z * ny + y) * nx + x;
          any |= D[i] != 0.0f;
          if (A) {
            const float4 a = A[i];
            any |= __float_as_uint(a.x) != b0 || __float_as_uint(a.y) != b1 || __float_as_uint(a.z) != b2 ||
                   __float_as_uint(a.w) != b3;
          }
        }
      }
    }
    // every lane of the workgroup gets here (the loop bounds are the workgroup's)
    any |= __shfl_xor(any, 1);
    any |= __shfl_xor(any, 2);
    any |= __shfl_xor(any, 4);
    const uint32_t lx = x >> 3;
    if ((x & 7u) == 0 && lx < lnx) flags[((size_t)lz * lny + ly) * lnx + lx] = any;
  }
}

// flags[leaf] = 1 iff the leaf or one of its 7 forward neighbours exists (it needs a cell leaf)
__global__ __launch_bounds__(256) void k_cell_leaf_flags(const uint32_t* __restrict__ table, uint32_t lnx, uint32_t lny,
                                                         uint32_t lnz, uint32_t* __restrict__ flags) {
  const size_t n = (size_t)lnx * lny * lnz;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const uint32_t x = (uint32_t)(i % lnx), y = (uint32_t)((i / lnx) % lny), z = (uint32_t)(i / ((size_t)lnx * lny));
    uint32_t any = 0;
    for (uint32_t dz = 0; dz < 2; ++dz)
      for (uint32_t dy = 0; dy < 2; ++dy)
        for (uint32_t dx = 0; dx < 2; ++dx)
          if (x + dx < lnx && y + dy < lny && z + dz < lnz)
            any |= table[((size_t)(z + dz) * lny + (y + dy)) * lnx + (x + dx)] != kNoLeaf;
    flags[i] = any;
  }
}

// --------------------------------------------------------- exclusive scan ---
// Of 0/1 flags, in three launches.  A workgroup owns a tile of kScanTile flags, which it takes in
// kScanSteps steps of 256 consecutive flags (item = tile base + step * 256 + work-item).

// One step: the number of set flags before this work-item's in the step; total: the step's count.
__device__ __forceinline__ uint32_t step_scan(bool f, uint32_t* s_w, uint32_t& total) {
  const unsigned long long b = __ballot(f);
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint32_t within = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
  if (lane == 0) s_w[w] = (uint32_t)__popcll(b);
  __syncthreads();
  uint32_t before = 0;
  total = 0;
  for (uint32_t k = 0; k < 4; ++k) {
    const uint32_t c = s_w[k];
    before += k < w ? c : 0u;
    total += c;
  }
  __syncthreads();  // s_w is written again by the next step
  return before + within;
}

__global__ __launch_bounds__(256) void k_tile_counts(const uint32_t* __restrict__ flags, size_t n,
                                                     uint32_t* __restrict__ sums) {
  const size_t base = (size_t)blockIdx.x * kScanTile;
  uint32_t cnt = 0;
  for (uint32_t k = 0; k < kScanSteps; ++k) {
    const size_t i = base + (size_t)k * 256 + threadIdx.x;
    cnt += i < n ? (flags[i] != 0u) : 0u;
  }
  cnt = wave_sum(cnt);
  __shared__ uint32_t s_w[4];
  if ((threadIdx.x & 63u) == 0) s_w[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) sums[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// One workgroup: sums[0..nb) -> their exclusive prefix sums in place, *total the sum of all.
__global__ __launch_bounds__(1024) void k_scan_sums(uint32_t* __restrict__ sums, uint32_t nb,
                                                    uint32_t* __restrict__ total) {
  __shared__ uint32_t s_w[16];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < nb; base += 1024u) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < nb ? sums[i] : 0u;
    uint32_t x = v;
    for (uint32_t o = 1; o < 64u; o <<= 1) {
      const uint32_t t = __shfl_up(x, o);
      if (lane >= o) x += t;
    }
    if (lane == 63u) s_w[w] = x;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t k = 0; k < 16u; ++k) {
      const uint32_t c = s_w[k];
      before += k < w ? c : 0u;
      all += c;
    }
    __syncthreads();
    if (i < nb) sums[i] = carry + before + x - v;
    carry += all;
  }
  if (threadIdx.x == 0) *total = carry;
}

// table[leaf] = its slot (the number of existing leaves before it) or CVR_NO_LEAF;
// slot_leaf[slot] = the leaf's index.
__global__ __launch_bounds__(256) void k_scatter_leaves(const uint32_t* __restrict__ flags, size_t n,
                                                        const uint32_t* __restrict__ sums,
                                                        uint32_t* __restrict__ table,
                                                        uint32_t* __restrict__ slot_leaf) {
  __shared__ uint32_t s_w[4];
  const size_t base = (size_t)blockIdx.x * kScanTile;
  uint32_t carry = sums[blockIdx.x];
  for (uint32_t k = 0; k < kScanSteps; ++k) {
    const size_t i = base + (size_t)k * 256 + threadIdx.x;
    const bool f = i < n && flags[i] != 0u;
    uint32_t total;
    const uint32_t slot = carry + step_scan(f, s_w, total);
    if (f) {
      table[i] = slot;
      slot_leaf[slot] = (uint32_t)i;
    } else if (i < n) {
      table[i] = kNoLeaf;
    }
    carry += total;
  }
}

// cell_slot[leaf] = 1 + the number of flagged leaves before it, or 0 (the zero leaf);
// coords[3 slot ..] = the leaf's coordinates; the leaf's super-brick bit of the mask (emask may be
// null: no mask), derived as cvr_set_medium_sparse does: bit (z >> k) << shz | (y >> k) << shy | x >> k.
__global__ __launch_bounds__(256) void k_scatter_cell_leaves(const uint32_t* __restrict__ flags, size_t n,
                                                             const uint32_t* __restrict__ sums, uint32_t lnx,
                                                             uint32_t lny, uint32_t* __restrict__ cell_slot,
                                                             uint32_t* __restrict__ coords, uint32_t* emask,
                                                             uint32_t k_shift, uint32_t shy, uint32_t shz) {
  __shared__ uint32_t s_w[4];
  const size_t base = (size_t)blockIdx.x * kScanTile;
  uint32_t carry = sums[blockIdx.x];
  if (blockIdx.x == 0 && threadIdx.x < 3u) coords[threadIdx.x] = 0u;  // slot 0: the zero leaf
  for (uint32_t k = 0; k < kScanSteps; ++k) {
    const size_t i = base + (size_t)k * 256 + threadIdx.x;
    const bool f = i < n && flags[i] != 0u;
    uint32_t total;
    const uint32_t slot = 1u + carry + step_scan(f, s_w, total);
    if (f) {
      const uint32_t x = (uint32_t)(i % lnx), y = (uint32_t)((i / lnx) % lny), z = (uint32_t)(i / ((size_t)lnx * lny));
      cell_slot[i] = slot;
      coords[3 * (size_t)slot] = x;
      coords[3 * (size_t)slot + 1] = y;
      coords[3 * (size_t)slot + 2] = z;
      if (emask) {
        const uint32_t b = (z >> k_shift) << shz | (y >> k_shift) << shy | (x >> k_shift);
        const uint32_t bit = 1u << (b & 31u);
        // (bits are only ever set: a stale read costs one atomic that changes nothing)
        if (!(__atomic_load_n(&emask[b >> 5], __ATOMIC_RELAXED) & bit)) atomicOr(&emask[b >> 5], bit);
      }
    } else if (i < n) {
      cell_slot[i] = 0u;
    }
    carry += total;
  }
}

// ----------------------------------------------------------------- gather ---
// Pool voxel p = slot * 512 + ((z & 7) * 8 + (y & 7)) * 8 + (x & 7) of every stored leaf: the
// grid's voxel, or (0, background) outside the grid; format 1 converts to binary16 here.
// kStore false: nothing is written; the smallest pool index (albedo: 4 p + channel) whose value
// overflows binary16 goes to out, the index cvr_set_medium_sparse would name.
template <bool kStore>
__global__ __launch_bounds__(256) void k_gather_leaves(const float* __restrict__ D, const float4* __restrict__ A,
                                                       uint32_t nx, uint32_t ny, uint32_t nz, uint32_t lnx,
                                                       uint32_t lny, const uint32_t* __restrict__ slot_leaf,
                                                       size_t n_pool, float4 bg, uint32_t format,
                                                       void* __restrict__ leaf_density, void* __restrict__ leaf_albedo,
                                                       MedScan* __restrict__ out) {
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n_pool; p += (size_t)gridDim.x * 256) {
    const uint32_t leaf = slot_leaf[p >> 9], local = (uint32_t)p & 511u;
    const uint32_t lx = leaf % lnx, ly = (leaf / lnx) % lny, lz = leaf / (lnx * lny);
    const uint32_t x = lx * 8u + (local & 7u), y = ly * 8u + ((local >> 3) & 7u), z = lz * 8u + (local >> 6);
    const bool in = x < nx && y < ny && z < nz;
    const size_t i = in ? ((size_t)z * ny + y) * nx + x : 0;
    const float d = in ? D[i] : 0.0f;
    if (kStore) {
      if (format)
        reinterpret_cast<_Float16*>(leaf_density)[p] = (_Float16)d;
      else
        reinterpret_cast<float*>(leaf_density)[p] = d;
    } else if (half_overflow(d)) {
      atomicMin(&out->ovf_density, (unsigned long long)p);
    }
    if (A) {
      const float4 a = in ? A[i] : bg;
      if (!kStore) {
        const unsigned long long at =
            half_overflow(a.x) ? 4 * p : half_overflow(a.y) ? 4 * p + 1 : half_overflow(a.z) ? 4 * p + 2 : kNoIndex;
        if (at != kNoIndex) atomicMin(&out->ovf_albedo, at);
      } else if (format) {
        uint2 h;
        h.x = half_bits(a.x) | half_bits(a.y) << 16;
        h.y = half_bits(a.z) | half_bits(a.w) << 16;
        reinterpret_cast<uint2*>(leaf_albedo)[p] = h;
      } else {
        reinterpret_cast<float4*>(leaf_albedo)[p] = a;
      }
    }
  }
}

uint32_t stream_grid(size_t n) { return (uint32_t)std::min<size_t>((n + 255) / 256, 8192); }
// the scans: 8 resident workgroups per CU of 256, each looping
uint32_t scan_grid(size_t n) { return (uint32_t)std::min<size_t>((n + 255) / 256, 2048); }

}  // namespace

hipError_t launch_scan_density(const float* density, size_t n, uint32_t format, MedScan* out, hipStream_t s) {
  hipLaunchKernelGGL(k_scan_density, dim3(scan_grid((n + 3) / 4)), dim3(256), 0, s, density, n, format, out);
  return hipGetLastError();
}

hipError_t launch_scan_albedo(const float* albedo, size_t n, uint32_t format, MedScan* out, hipStream_t s) {
  hipLaunchKernelGGL(k_scan_albedo, dim3(scan_grid(n)), dim3(256), 0, s, reinterpret_cast<const float4*>(albedo), n,
                     format, out);
  return hipGetLastError();
}

hipError_t launch_fill_albedo(void* albedo, size_t n, uint32_t format, const float value[4], hipStream_t s) {
  hipLaunchKernelGGL(k_fill_albedo, dim3(stream_grid(n)), dim3(256), 0, s, albedo, n, format,
                     make_float4(value[0], value[1], value[2], value[3]));
  return hipGetLastError();
}

hipError_t launch_leaf_flags(const float* density, const float* albedo, const uint32_t res[3], const uint32_t ln[3],
                             uint32_t* flags, hipStream_t s) {
  const size_t ntasks = (size_t)((ln[0] + 31u) / 32u) * ln[1] * ln[2];
  hipLaunchKernelGGL(k_leaf_flags, dim3((uint32_t)std::min<size_t>(ntasks, 1u << 20)), dim3(256), 0, s, density,
                     reinterpret_cast<const float4*>(albedo), res[0], res[1], res[2], ln[0], ln[1], ln[2], flags);
  return hipGetLastError();
}

hipError_t launch_cell_leaf_flags(const uint32_t* table, const uint32_t ln[3], uint32_t* flags, hipStream_t s) {
  hipLaunchKernelGGL(k_cell_leaf_flags, dim3(stream_grid((size_t)ln[0] * ln[1] * ln[2])), dim3(256), 0, s, table,
                     ln[0], ln[1], ln[2], flags);
  return hipGetLastError();
}

size_t flag_scan_tiles(size_t n) { return (n + kScanTile - 1) / kScanTile; }

hipError_t launch_flag_scan(const uint32_t* flags, size_t n, uint32_t* sums, uint32_t* total, hipStream_t s) {
  const uint32_t nb = (uint32_t)flag_scan_tiles(n);
  hipLaunchKernelGGL(k_tile_counts, dim3(nb), dim3(256), 0, s, flags, n, sums);
  hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, s, sums, nb, total);
  return hipGetLastError();
}

hipError_t launch_scatter_leaves(const uint32_t* flags, size_t n, const uint32_t* sums, uint32_t* table,
                                 uint32_t* slot_leaf, hipStream_t s) {
  hipLaunchKernelGGL(k_scatter_leaves, dim3((uint32_t)flag_scan_tiles(n)), dim3(256), 0, s, flags, n, sums, table,
                     slot_leaf);
  return hipGetLastError();
}

hipError_t launch_scatter_cell_leaves(const uint32_t* flags, size_t n, const uint32_t* sums, const uint32_t ln[3],
                                      uint32_t* cell_slot, uint32_t* coords, uint32_t* emask, uint32_t k_shift,
                                      uint32_t shy, uint32_t shz, hipStream_t s) {
  hipLaunchKernelGGL(k_scatter_cell_leaves, dim3((uint32_t)flag_scan_tiles(n)), dim3(256), 0, s, flags, n, sums, ln[0],
                     ln[1], cell_slot, coords, emask, k_shift, shy, shz);
  return hipGetLastError();
}

hipError_t launch_gather_leaves(const float* density, const float* albedo, const uint32_t res[3], const uint32_t ln[3],
                                const uint32_t* slot_leaf, size_t n_leaves, const float bg[4], uint32_t format,
                                void* leaf_density, void* leaf_albedo, MedScan* check, hipStream_t s) {
  const size_t np = n_leaves * 512;
  if (np == 0) return hipSuccess;
  const float4 b = make_float4(bg[0], bg[1], bg[2], bg[3]);
  const float4* A = reinterpret_cast<const float4*>(albedo);
  if (check)
    hipLaunchKernelGGL(k_gather_leaves<false>, dim3(stream_grid(np)), dim3(256), 0, s, density, A, res[0], res[1],
                       res[2], ln[0], ln[1], slot_leaf, np, b, format, nullptr, nullptr, check);
  else
    hipLaunchKernelGGL(k_gather_leaves<true>, dim3(stream_grid(np)), dim3(256), 0, s, density, A, res[0], res[1],
                       res[2], ln[0], ln[1], slot_leaf, np, b, format, leaf_density, leaf_albedo, nullptr);
  return hipGetLastError();
}

}  // namespace cvr
