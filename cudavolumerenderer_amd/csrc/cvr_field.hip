// Field statistics and value-gradient histograms of a scalar field in device memory
// (cvr_field_stats, cvr_field_histogram; cvr.h states what is computed, cvr_kernels.h holds the
// one definition of the bin rule, cvr_gradient.h that of u, v and the gradient).  Every result is
// an integer count or an order-independent extremum, so any schedule returns the host statement's
// numbers exactly.
//
// The 2-D histogram and the statistics need the gradient: k_field_walk runs gradient_walk
// (cvr_gradient.h), the walk k_gradient (cvr_medium_build.hip) classifies from, and bins or scans
// what it hands over.  The 1-D histogram has no stencil and streams the field 16 bytes per lane.
//
// A workgroup keeps its histogram in LDS (sized to the bins it holds, not to the limit, so that
// small tables leave the CU its occupancy), updates it with non-returning LDS adds and flushes it
// once with one global add per non-zero bin.  More than kFieldLdsBins bins (up to 65536, 256 KB)
// do not fit: they are cut into 2 to 4 equal bands of consecutive bins, and blockIdx.y names the
// band a workgroup counts; it walks the whole field and drops the voxels of the other bands.  The
// bands of one launch run side by side and share the field's lines in L2.  Adding straight into
// the output with global atomics instead took 16.5 ms on C2's grid, where 77 % of the voxels fall
// into one bin and the adds to it serialise at the memory side, against 0.6 ms on a uniform random
// field (profiles/histogram/README.md); the bands cost the same on both.
// Equal bins are merged across the wave before the add (add_merged below).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "cvr_device.h"
#include "cvr_kernels.h"

// 0: every lane adds its own 1 (the A/B partner of the merge, profiles/histogram/README.md)
#ifndef CVR_FIELD_MERGE
#define CVR_FIELD_MERGE 1
#endif

namespace cvr {
namespace {

// hist[bin] += 1 for every lane with `active`; every lane of the wave calls this.  The lanes that
// hold the first active lane's bin are counted by a ballot and added by that lane alone (a wave
// inside one material: one add of up to 64); the other lanes add their own.  The result of the
// add is not used, so it is a non-returning atomic.
__device__ __forceinline__ void add_merged(uint32_t* hist, uint32_t bin, bool active) {
#if CVR_FIELD_MERGE
  const unsigned long long act = __ballot(active);
  if (act == 0ull) return;  // (wave-uniform)
  const uint32_t first = (uint32_t)__ffsll((long long)act) - 1u;
  const uint32_t b0 = __shfl(bin, first);
  const unsigned long long same = __ballot(active && bin == b0);
  const uint32_t lane = threadIdx.x & 63u;
  if (lane == first)
    atomicAdd(&hist[b0], (uint32_t)__popcll(same));
  else if (active && bin != b0)
    atomicAdd(&hist[bin], 1u);
#else
  if (active) atomicAdd(&hist[bin], 1u);
#endif
}

// The workgroup's band of the histogram: bins [lo, lo + n) of `bins`, n <= band, in LDS.
struct Band {
  uint32_t lo, n;
  uint32_t* hist;
  // (cleared here, flushed by flush(); every work-item of the workgroup calls both)
  __device__ __forceinline__ Band(uint32_t bins, uint32_t band) {
    extern __shared__ uint32_t s_hist[];
    lo = blockIdx.y * band;
    n = bins - lo < band ? bins - lo : band;
    hist = s_hist;
    for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) s_hist[k] = 0u;
    __syncthreads();
  }
  // one voxel of bin `bin` (of all bins) in every lane with `active`; every lane of the wave calls this
  __device__ __forceinline__ void add(uint32_t bin, bool active) { add_merged(hist, bin - lo, active && bin - lo < n); }
  __device__ __forceinline__ void flush(uint32_t* __restrict__ counts) {
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) {
      const uint32_t v = hist[k];
      if (v) atomicAdd(&counts[lo + k], v);
    }
  }
};

// What a work-item has seen for the statistics; commit() reduces the workgroup's into out with at
// most one atomic of each kind, and none where out already holds what the workgroup found.
struct StatScan {
  uint32_t kmin = kFieldKeyPosInf, kmax = kFieldKeyNegInf, gmax = 0u, nan_v = 0u, nan_g = 0u;
  __device__ __forceinline__ void take(float s, float mag) {
    if (s == s) {
      const uint32_t k = field_key(__float_as_uint(s));
      kmin = k < kmin ? k : kmin;
      kmax = k > kmax ? k : kmax;
    } else {
      ++nan_v;
    }
    if (mag == mag) {
      // mag >= +0, so its bits order as the values do
      const uint32_t g = __float_as_uint(mag);
      gmax = g > gmax ? g : gmax;
    } else {
      ++nan_g;
    }
  }
  __device__ __forceinline__ void commit(FieldScan* __restrict__ out) {
    __shared__ uint32_t s_red[4][5];
    kmin = wave_min(kmin);
    kmax = wave_max(kmax);
    gmax = wave_max(gmax);
    // (a work-item's counts and a wave's sums stay below 2^32: the field has fewer voxels)
    nan_v = wave_sum(nan_v);
    nan_g = wave_sum(nan_g);
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (lane == 0) {
      s_red[w][0] = kmin, s_red[w][1] = kmax, s_red[w][2] = gmax, s_red[w][3] = nan_v, s_red[w][4] = nan_g;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long nv = nan_v, ng = nan_g;
      for (uint32_t k = 1; k < 4; ++k) {
        kmin = s_red[k][0] < kmin ? s_red[k][0] : kmin;
        kmax = s_red[k][1] > kmax ? s_red[k][1] : kmax;
        gmax = s_red[k][2] > gmax ? s_red[k][2] : gmax;
        nv += s_red[k][3];
        ng += s_red[k][4];
      }
      if (kmin < __atomic_load_n(&out->kmin, __ATOMIC_RELAXED)) atomicMin(&out->kmin, kmin);
      if (kmax > __atomic_load_n(&out->kmax, __ATOMIC_RELAXED)) atomicMax(&out->kmax, kmax);
      if (gmax > __atomic_load_n(&out->gmax_bits, __ATOMIC_RELAXED)) atomicMax(&out->gmax_bits, gmax);
      if (nv) atomicAdd(&out->nan_values, nv);
      if (ng) atomicAdd(&out->nan_gradients, ng);
    }
  }
};

// The stencil pass over gradient_walk (cvr_gradient.h).  kHist: the histogram of blockIdx.y's band
// of `band` bins into counts, merged across the wave, so every lane bins; otherwise the statistics
// of the lanes inside the row into out.
template <class T, bool kHist>
__global__ __launch_bounds__(256) void k_field_walk(const T* __restrict__ S, uint32_t nx, uint32_t ny, uint32_t nz,
                                                    GradientAxes axes, FieldBins b, uint32_t band,
                                                    uint32_t* __restrict__ counts, FieldScan* __restrict__ out) {
  Band hist(kHist ? b.n * b.m : 0u, band);
  StatScan st;
  gradient_walk(S, nx, ny, nz, axes, [&](bool in, uint32_t, uint32_t, uint32_t, float cur, float mag) {
    if constexpr (kHist) {
      const uint32_t i = field_bin(unit_clamp(cur, b.lo, b.hi), b.n);
      const uint32_t j = field_bin(unit_clamp(mag, b.glo, b.ghi), b.m);
      hist.add(j * b.n + i, in);
    } else {
      if (in) st.take(cur, mag);
    }
  });
  if constexpr (kHist)
    hist.flush(counts);
  else
    st.commit(out);
}

// The 1-D histogram.  Integer fields are cut as k_classified cuts them: a head up to the first
// 16-byte boundary, whole 16-byte groups (one per lane and trip: 1 KiB per wave and load), and a
// tail; head and tail (a float field: every voxel) are taken one voxel per lane.  The order of
// the voxels does not matter to a count, so a lane bins the voxels of its own group.
template <class T>
__global__ __launch_bounds__(256) void k_field_hist1d(const T* __restrict__ S, size_t n, FieldBins b, uint32_t band,
                                                      uint32_t* __restrict__ counts) {
  Band hist(b.n, band);
  constexpr uint32_t kSize = (uint32_t)sizeof(T), V = kSize < 4u ? 16u / kSize : 1u;
  const uint32_t lane = threadIdx.x & 63u;
  size_t head = 0, body_end = 0;
  if constexpr (V > 1u) {
    head = ((16u - (uint32_t)((uintptr_t)S & 15u)) & 15u) / kSize;
    head = head < n ? head : n;
    const size_t groups = (n - head) / V;
    body_end = head + groups * V;
    const uint4* __restrict__ S16 = reinterpret_cast<const uint4*>(S + head);
    const size_t wave = ((size_t)blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (size_t)gridDim.x * 4;
    // (the bounds are the wave's: every lane takes part in the merge)
    for (size_t g0 = wave * 64; g0 < groups; g0 += nwaves * 64) {
      const bool active = g0 + lane < groups;
      const uint4 q = active ? S16[g0 + lane] : make_uint4(0u, 0u, 0u, 0u);
      const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (uint32_t k = 0; k < V; ++k) {
        const uint32_t byte = k * kSize;
        const T v = (T)(w[byte >> 2] >> ((byte & 3u) * 8u));
        hist.add(field_bin(unit_clamp((float)v, b.lo, b.hi), b.n), active);
      }
    }
  }
  const size_t rest = head + (n - body_end);
  for (size_t e0 = (size_t)blockIdx.x * 256 + (threadIdx.x & ~63u); e0 < rest; e0 += (size_t)gridDim.x * 256) {
    const size_t e = e0 + lane;
    const bool active = e < rest;
    const size_t i = !active ? 0 : e < head ? e : body_end + (e - head);
    hist.add(field_bin(unit_clamp((float)S[i], b.lo, b.hi), b.n), active);
  }
  hist.flush(counts);
}

// A grid of at most `cap` workgroups (per band) over `work` workgroup-sized pieces.  A workgroup
// flushes the `lds_bins` words of its histogram (0: none), so it gets at least that many voxels:
// the flush then costs no more than the pass (G workgroups flush at most G * lds_bins <= voxels
// words).  Eight or more are rounded down to the XCDs' multiple (the walk's turn of the block index
// needs it).
uint32_t field_grid(size_t work, size_t voxels, uint32_t lds_bins, uint32_t cap) {
  size_t g = std::min<size_t>(work, cap);
  if (lds_bins) g = std::min(g, std::max<size_t>(voxels / lds_bins, 1));
  g = std::max<size_t>(g, 1);
  return (uint32_t)(g >= 8 ? g & ~(size_t)7 : g);
}

template <class F>
hipError_t with_type(uint32_t scalar_type, F f) {
  switch (scalar_type) {
    case 0: return f((const float*)nullptr);
    case 1: return f((const uint8_t*)nullptr);
    case 2: return f((const uint16_t*)nullptr);
    case 3: return f((const int16_t*)nullptr);
    default: return hipErrorInvalidValue;
  }
}

size_t walk_tasks(const FieldSrc& f) { return gradient_walk_tasks(f.res[0], f.res[1], f.res[2]); }

}  // namespace

hipError_t launch_field_stats(const FieldSrc& f, FieldScan* d_out, hipStream_t s) {
  const size_t voxels = (size_t)f.res[0] * f.res[1] * f.res[2];
  const uint32_t grid = field_grid(walk_tasks(f), voxels, 0u, kWalkTaskCap);
  return with_type(f.scalar_type, [&](auto* tag) {
    using T = std::remove_cv_t<std::remove_pointer_t<decltype(tag)>>;
    hipLaunchKernelGGL((k_field_walk<T, false>), dim3(grid), dim3(256), 0, s, static_cast<const T*>(f.scalar),
                       f.res[0], f.res[1], f.res[2], f.axes, FieldBins{}, 0u, (uint32_t*)nullptr, d_out);
    return hipGetLastError();
  });
}

hipError_t launch_field_histogram(const FieldSrc& f, const FieldBins& b, uint32_t* d_counts, hipStream_t s) {
  const size_t voxels = (size_t)f.res[0] * f.res[1] * f.res[2];
  const uint32_t bins = b.n * b.m;
  // equal bands of at most kFieldLdsBins bins: one up to the limit, four at 65536
  const uint32_t nbands = (bins + kFieldLdsBins - 1u) / kFieldLdsBins, band = (bins + nbands - 1u) / nbands;
  const size_t lds_bytes = (size_t)band * sizeof(uint32_t);
  if (hipError_t e = hipMemsetAsync(d_counts, 0, (size_t)bins * sizeof(uint32_t), s)) return e;
  return with_type(f.scalar_type, [&](auto* tag) {
    using T = std::remove_cv_t<std::remove_pointer_t<decltype(tag)>>;
    const T* S = static_cast<const T*>(f.scalar);
    if (b.m > 1u) {
      const uint32_t grid = field_grid(walk_tasks(f), voxels, band, kWalkTaskCap);
      hipLaunchKernelGGL((k_field_walk<T, true>), dim3(grid, nbands), dim3(256), lds_bytes, s, S, f.res[0], f.res[1],
                         f.res[2], f.axes, b, band, d_counts, (FieldScan*)nullptr);
    } else {
      // a workgroup's trip: 256 lanes of 16 bytes (a float field: of one voxel)
      const size_t per_trip = 256u * (sizeof(T) < 4 ? 16u / sizeof(T) : 1u);
      const uint32_t grid = field_grid((voxels + per_trip - 1) / per_trip, voxels, band, kFieldGrid1D);
      hipLaunchKernelGGL((k_field_hist1d<T>), dim3(grid, nbands), dim3(256), lds_bytes, s, S, voxels, b, band, d_counts);
    }
    return hipGetLastError();
  });
}

}  // namespace cvr
