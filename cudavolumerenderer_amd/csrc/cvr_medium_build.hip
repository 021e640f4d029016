// cvr_medium_build.hip - the device-side front end of cvr_set_medium_device,
// cvr_set_medium_scalar and cvr_set_medium_gradient (gfx950): what the host uploads decide with
// loops over every voxel or leaf, decided here from a voxel source in device memory, the caller's
// two arrays or a scalar field classified through a transfer table staged in LDS (1-D by the
// value, 2-D by the value and the gradient magnitude of a 6-neighbour stencil, or one row per
// label byte of a label volume).  Value scans
// (majorant, binary16 overflow, uniform albedo), the dense -> 8^3 leaves
// rule of cvr.h (leaf flags, exclusive scan, gather), the cell-leaf table and the empty-region
// mask.  The cells, bounds and brick words are then built by cvr_kernels.hip's kernels, unchanged.
// A source may stand behind a clip region (cvr.h: CVR_HAS_CLIP; Clipped below): the same stages
// then run clipped instances, and a context without a clip runs the ones it always ran.
//
// No kernel here waits on another workgroup: the exclusive scan is three launches (per-tile
// counts, one workgroup over the tile sums, scatter), ordered by the stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "cvr_device.h"
#include "cvr_host.h"
#include "cvr_kernels.h"

namespace cvr {
namespace {

constexpr uint32_t kNoLeaf = 0xFFFFFFFFu;  // CVR_NO_LEAF
constexpr unsigned long long kNoIndex = ~0ull;

// finite and rounds to +-inf in binary16 (the host uploads' half_overflows)
__device__ __forceinline__ bool half_overflow(float f) {
  const float a = fabsf(f);
  return a >= 65520.0f && a < __builtin_huge_valf();
}
__device__ __forceinline__ uint32_t half_bits(float f) {
  const _Float16 h = (_Float16)f;
  return (uint32_t)__builtin_bit_cast(unsigned short, h);
}
// a float4's four components as binary16, round to nearest even: the half format's albedo voxel
__device__ __forceinline__ uint2 half4_bits(const float4 a) {
  uint2 h;
  h.x = half_bits(a.x) | half_bits(a.y) << 16;
  h.y = half_bits(a.z) | half_bits(a.w) << 16;
  return h;
}

// ---------------------------------------------------------- voxel sources ---
// Where a kernel takes a voxel's density and albedo from.  The caller's two arrays:
struct ArraySrc {
  using Scalar = void;
  const float* __restrict__ D;
  const float4* __restrict__ A;  // null: no albedo
  __device__ void stage() {}
  __device__ bool has_albedo() const { return A != nullptr; }
  __device__ void voxel(size_t i, float& d, float4& a) const {
    d = D[i];
    if (A) a = A[i];
  }
  // (the leaf kernels name a voxel by its coordinates too: only a stencil needs them)
  __device__ void voxel(uint32_t, uint32_t, uint32_t, size_t i, float& d, float4& a) const { voxel(i, d, a); }
};
// A scalar field of type T classified through the transfer table (cvr.h; transfer_classify is the
// statement).  stage() copies the table into the workgroup's dynamic LDS, n x 16 bytes, once;
// every work-item of the workgroup calls it before the first voxel().
template <class T>
struct ScalarSrc {
  using Scalar = T;
  const T* __restrict__ S;
  const float4* __restrict__ table;
  TransferParams p;
  uint32_t albedo;  // 0: the colours are not looked at (has_albedo() false)
  const float4* lds;
  __device__ void stage() {
    extern __shared__ float4 s_table[];
    for (uint32_t k = threadIdx.x; k < p.n; k += blockDim.x) s_table[k] = table[k];
    __syncthreads();
    lds = s_table;
  }
  __device__ bool has_albedo() const { return albedo != 0u; }
  __device__ void classified(float s, float& d, float4& a) const {
    const float4 e = transfer_classify(s, lds, p);
    d = e.w;
    a = make_float4(e.x, e.y, e.z, 1.0f);
  }
  __device__ void voxel(size_t i, float& d, float4& a) const { classified((float)S[i], d, a); }
  __device__ void voxel(uint32_t, uint32_t, uint32_t, size_t i, float& d, float4& a) const { voxel(i, d, a); }
};
// A scalar field of type T classified through the 2-D table by its value and its gradient
// magnitude (cvr.h; gradient_magnitude and gradient_classify are the statement).  stage() copies
// the m x n table into the workgroup's dynamic LDS once.  voxel() reads the voxel and its up to
// six in-grid neighbours from the field, wherever they lie: the gradient is the field's.
template <class T>
struct GradientSrc {
  using Scalar = T;
  const T* __restrict__ S;
  const float4* __restrict__ table;
  GradientParams p;
  uint32_t res[3];
  uint32_t albedo;  // 0: the colours are not looked at (has_albedo() false)
  const float4* lds;
  __device__ void stage() {
    extern __shared__ float4 s_table[];
    for (uint32_t k = threadIdx.x; k < p.n * p.m; k += blockDim.x) s_table[k] = table[k];
    __syncthreads();
    lds = s_table;
  }
  __device__ bool has_albedo() const { return albedo != 0u; }
  __device__ void classified(float s, float mag, float& d, float4& a) const {
    const float4 e = gradient_classify(s, mag, lds, p);
    d = e.w;
    a = make_float4(e.x, e.y, e.z, 1.0f);
  }
  __device__ void voxel(uint32_t x, uint32_t y, uint32_t z, size_t i, float& d, float4& a) const {
    const float mag = gradient_at([&](size_t at) { return (float)S[at]; }, x, y, z, res, p.axes);
    classified((float)S[i], mag, d, a);
  }
};
// A scalar field of type T and a label volume of one byte per voxel, classified through a table
// of m rows of p.n entries: the voxel's label byte chooses the row, row 0 for a byte the table has
// no row for (cvr.h: CVR_HAS_LABELS; label_classify is the statement).  stage() copies the m x n
// table into the workgroup's dynamic LDS once.  L may have any alignment.
template <class T>
struct LabeledSrc {
  using Scalar = T;
  const T* __restrict__ S;
  const uint8_t* __restrict__ L;
  const float4* __restrict__ table;
  TransferParams p;
  uint32_t m;
  uint32_t* __restrict__ counts;  // kLabelSlots x 256 words (VoxelSource::label_counts)
  uint32_t albedo;  // 0: the colours are not looked at (has_albedo() false)
  const float4* lds;
  __device__ void stage() {
    extern __shared__ float4 s_table[];
    for (uint32_t k = threadIdx.x; k < p.n * m; k += blockDim.x) s_table[k] = table[k];
    __syncthreads();
    lds = s_table;
  }
  __device__ bool has_albedo() const { return albedo != 0u; }
  __device__ void classified(float s, uint32_t label, float& d, float4& a) const {
    const float4 e = label_classify(s, label, lds, m, p);
    d = e.w;
    a = make_float4(e.x, e.y, e.z, 1.0f);
  }
  __device__ void voxel(size_t i, float& d, float4& a) const { classified((float)S[i], L[i], d, a); }
  __device__ void voxel(uint32_t, uint32_t, uint32_t, size_t i, float& d, float4& a) const { voxel(i, d, a); }
};
// a or, for a clipped voxel, a0, by component (a select of the two float4 objects would be a select
// of their addresses, and a0's is the kernel's by-value argument: it would be copied to scratch)
__device__ __forceinline__ float4 keep_or(bool keep, const float4 a, const float4 a0) {
  return make_float4(keep ? a.x : a0.x, keep ? a.y : a0.y, keep ? a.z : a0.z, keep ? a.w : a0.w);
}
// Any of the three behind a clip region (cvr_clip.h; cvr.h states the clipped voxel): the region
// travels with the source, by value, and so does a0, the unclipped source's albedo of voxel 0,
// which every clipped voxel gets (the host reads or classifies it once: source_voxel, whose bits
// are the kernels').  voxel() reads the source's voxel and then applies the test as a select, so
// the loads of an unrolled loop still issue together (a test before the load put every load
// behind a branch of its own); what is provably clipped is left unread by the kernels, a task or
// a wave at a time.  A kept voxel is the source's, a gradient source's stencil reading its
// neighbours from the field, clipped or not.
template <class Src>
struct Clipped {
  using Scalar = typename Src::Scalar;
  Src s;
  ClipRegion r;
  float4 a0;
  __device__ void stage() { s.stage(); }
  __device__ bool has_albedo() const { return s.has_albedo(); }
  __device__ bool keeps(uint32_t x, uint32_t y, uint32_t z) const { return clip_keeps(r, x, y, z); }
  // returns whether the voxel is kept
  __device__ bool voxel(uint32_t x, uint32_t y, uint32_t z, size_t i, float& d, float4& a) const {
    s.voxel(x, y, z, i, d, a);
    const bool keep = keeps(x, y, z);
    d = keep ? d : 0.0f;
    a = keep_or(keep, a, a0);
    return keep;
  }
};
template <class Src>
struct is_clipped : std::false_type {};
template <class Src>
struct is_clipped<Clipped<Src>> : std::true_type {};
// the labelled source of a source that has one, clipped or not
template <class Src>
struct is_labeled : std::false_type {};
template <class T>
struct is_labeled<LabeledSrc<T>> : std::true_type {};
template <class T>
struct is_labeled<Clipped<LabeledSrc<T>>> : std::true_type {};
template <class T>
__device__ __forceinline__ const LabeledSrc<T>& labeled(const LabeledSrc<T>& s) { return s; }
template <class T>
__device__ __forceinline__ const LabeledSrc<T>& labeled(const Clipped<LabeledSrc<T>>& s) { return s.s; }
// A work-item's count of kept voxels into out->kept: the workgroup's sum through LDS, then one
// atomic per workgroup that kept any, on one of kKeptSlots words by the workgroup's index (16 384
// atomics on a single word, one per wave of a 4096-workgroup launch, cost more than the pass they
// closed; the host adds the slots).  Every work-item of the workgroup calls it, once, at the end.
__device__ __forceinline__ void commit_kept(uint32_t kept, MedScan* __restrict__ out) {
  __shared__ uint32_t s_kept[4];
  const uint32_t w = wave_sum(kept);
  __syncthreads();  // (the table's LDS or a scan's scratch is not touched: s_kept is its own)
  if ((threadIdx.x & 63u) == 0) s_kept[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t all = s_kept[0] + s_kept[1] + s_kept[2] + s_kept[3];
    if (all) atomicAdd(&out->kept[blockIdx.x % kKeptSlots], (unsigned long long)all);
  }
}

// 0: the label counters compiled out (the A/B partner, profiles/labels/README.md)
#ifndef CVR_LABEL_COUNTS
#define CVR_LABEL_COUNTS 1
#endif
// The kept voxels per label byte of a labelled build: 256 counters in the workgroup's LDS, beside
// the table's, and at the workgroup's end one global add per counter that is not zero, into the
// copy of the 256 words that the workgroup's index names (the host adds the kLabelSlots copies).
// No voxel and no wave adds to global memory (cvr_field.hip and commit_kept record what that costs).
// Integer adds: the result does not depend on their order.
struct LabelCounts {
  uint32_t* s;
  // every work-item of the workgroup, before stage(), whose barrier orders the zeroes
  __device__ __forceinline__ void begin() {
    __shared__ uint32_t s_counts[256];
    s = s_counts;
    for (uint32_t k = threadIdx.x; k < 256u; k += blockDim.x) s_counts[k] = 0u;
  }
  // one voxel of label byte `label` in every lane with `active`.  Label volumes are mostly one
  // label: the lanes that hold the first active lane's label are counted by a ballot and added by
  // that lane alone, as the field histogram merges its bins; the other lanes add their own.  (The
  // ballots are of the lanes that get here.)
  __device__ __forceinline__ void add(uint32_t label, bool active) {
#if CVR_LABEL_COUNTS
    const unsigned long long act = __ballot(active);
    if (act == 0ull) return;  // (wave-uniform)
    const uint32_t first = (uint32_t)__ffsll((long long)act) - 1u;
    // (first is the wave's: a lane read, not a shuffle)
    const uint32_t l0 = (uint32_t)__builtin_amdgcn_readlane((int)label, __builtin_amdgcn_readfirstlane((int)first));
    const unsigned long long same = __ballot(active && label == l0);
    if ((threadIdx.x & 63u) == first)
      atomicAdd(&s[l0], (uint32_t)__popcll(same));
    else if (active && label != l0)
      atomicAdd(&s[label], 1u);
#else
    (void)label, (void)active;
#endif
  }
  // every work-item of the workgroup, once, after its last add
  __device__ __forceinline__ void flush(uint32_t* __restrict__ counts) {
#if CVR_LABEL_COUNTS
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < 256u; k += blockDim.x) {
      const uint32_t v = s[k];
      if (v) atomicAdd(&counts[(blockIdx.x % kLabelSlots) * 256u + k], v);
    }
#else
    (void)counts;
#endif
  }
};

// ----------------------------------------------------------- value scans ---
// Streaming reads: consecutive lanes read consecutive 16 bytes (1 KiB per wave and load), a wave
// reduction, then at most one atomic of each kind per workgroup, and none when the result already
// holds what the workgroup found (the values only grow, fall or gain bits, so a stale read costs an
// atomic that changes nothing).  Atomics on one word are serialised at the memory side: with 8192
// workgroups each issuing theirs, C2's 60 MB density scan took 0.095 ms; with 2048 workgroups and
// the reads first, 0.026 ms (profiles/device_medium/README.md).

// What a work-item has seen of the densities; commit() reduces the workgroup's (s_mx, s_ov: 4
// entries of LDS each) into out.
struct DensityScan {
  float mx = 0.0f;  // max(0, every non-NaN voxel): a NaN or -0 never compares greater
  unsigned long long ov = kNoIndex;
  __device__ __forceinline__ void take(float v, size_t i, uint32_t format) {
    mx = v > mx ? v : mx;
    if (format && half_overflow(v) && i < ov) ov = i;
  }
  __device__ __forceinline__ void commit(float* s_mx, unsigned long long* s_ov, MedScan* __restrict__ out) {
    mx = wave_max(mx);
    ov = wave_min(ov);
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
};
// The same of the albedos, against voxel 0's.  albedo_flags bit 0: some voxel's rgb differs from
// voxel 0's (format 1: the rounded halves; bits are compared, w is ignored); bit 1: some voxel's
// 16 bytes differ from voxel 0's (the leaf rule).
struct AlbedoScan {
  uint32_t f0, f1, f2, f3, h0, h1, h2;
  uint32_t flags = 0;
  unsigned long long ov = kNoIndex;
  __device__ __forceinline__ explicit AlbedoScan(const float4 f)
      : f0(__float_as_uint(f.x)), f1(__float_as_uint(f.y)), f2(__float_as_uint(f.z)), f3(__float_as_uint(f.w)),
        h0(half_bits(f.x)), h1(half_bits(f.y)), h2(half_bits(f.z)) {}
  __device__ __forceinline__ void take(const float4 a, size_t i, uint32_t format) {
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
  __device__ __forceinline__ void commit(uint32_t* s_fl, unsigned long long* s_ov, MedScan* __restrict__ out) {
    flags = wave_or(flags);
    ov = wave_min(ov);
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
};

__global__ __launch_bounds__(256) void k_scan_density(const float* __restrict__ D, size_t n, uint32_t format,
                                                      MedScan* __restrict__ out) {
  DensityScan ds;
  // 16 bytes per lane where the array's alignment allows it, the last n % 4 voxels one by one
  const size_t n4 = ((uintptr_t)D & 15u) ? 0 : n / 4;
  const float4* __restrict__ D4 = reinterpret_cast<const float4*>(D);
#pragma unroll 2
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const float4 v = D4[i];
    ds.take(v.x, 4 * i, format);
    ds.take(v.y, 4 * i + 1, format);
    ds.take(v.z, 4 * i + 2, format);
    ds.take(v.w, 4 * i + 3, format);
  }
  for (size_t i = 4 * n4 + (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    ds.take(D[i], i, format);
  __shared__ float s_mx[4];
  __shared__ unsigned long long s_ov[4];
  ds.commit(s_mx, s_ov, out);
}

__global__ __launch_bounds__(256) void k_scan_albedo(const float4* __restrict__ A, size_t n, uint32_t format,
                                                     MedScan* __restrict__ out) {
  AlbedoScan as(A[0]);
#pragma unroll 2
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) as.take(A[i], i, format);
  __shared__ uint32_t s_fl[4];
  __shared__ unsigned long long s_ov[4];
  as.commit(s_fl, s_ov, out);
}

// Both scans' workgroup reductions with the table's LDS as their scratch, after the workgroup's
// last voxel (the launches allocate at least 8 entries).
__device__ __forceinline__ void commit_in_table_lds(DensityScan& ds, AlbedoScan& as, MedScan* __restrict__ out) {
  extern __shared__ float4 s_table[];
  __syncthreads();  // the table is read no more
  unsigned long long* s_ov = reinterpret_cast<unsigned long long*>(s_table);
  float* s_mx = reinterpret_cast<float*>(s_ov + 8);
  ds.commit(s_mx, s_ov, out);
  as.commit(reinterpret_cast<uint32_t*>(s_mx + 4), s_ov + 4, out);
}

// What both classified passes do with voxel i's density d and albedo a.  kStore false: the scan,
// which finds what k_scan_density and k_scan_albedo find, of the classified values, together.
// kStore true: the voxel into the context's grids (format 1: as binary16).
template <bool kStore>
__device__ __forceinline__ void emit(size_t i, float d, const float4 a, uint32_t format, DensityScan& ds,
                                     AlbedoScan& as, void* __restrict__ density, void* __restrict__ albedo) {
  if (!kStore) {
    ds.take(d, i, format);
    as.take(a, i, format);
  } else if (format) {
    reinterpret_cast<_Float16*>(density)[i] = (_Float16)d;
    reinterpret_cast<uint2*>(albedo)[i] = half4_bits(a);
  } else {
    reinterpret_cast<float*>(density)[i] = d;
    reinterpret_cast<float4*>(albedo)[i] = a;
  }
}

// The classified source's two dense passes over the scalar field (kStore: emit above).  Integer
// scalars are loaded 16 bytes per lane: the field is cut into a head up to the first 16-byte
// boundary, whole 16-byte groups, and a tail; a wave loads 64 groups (1 KiB) and hands the
// voxels round with lane shuffles so that in each of its V steps lane l has voxel 64 k + l of the
// wave's run, and the stores of a step are consecutive.  Head and tail (a float field: every
// voxel) are taken one voxel per lane.  The workgroup reduction's scratch is the table's LDS, after
// the last voxel (at least 8 entries are allocated).
template <class T, bool kStore>
__global__ __launch_bounds__(256) void k_classified(ScalarSrc<T> src, size_t n, uint32_t format,
                                                    void* __restrict__ density, void* __restrict__ albedo,
                                                    MedScan* __restrict__ out) {
  src.stage();
  float d0;
  float4 a0;
  src.voxel(0, d0, a0);
  DensityScan ds;
  AlbedoScan as(a0);
  auto take = [&](size_t i, float s) {
    float d;
    float4 a;
    src.classified(s, d, a);
    emit<kStore>(i, d, a, format, ds, as, density, albedo);
  };
  constexpr uint32_t kSize = (uint32_t)sizeof(T), V = kSize < 4u ? 16u / kSize : 1u;
  size_t head = 0, body_end = 0;
  if constexpr (V > 1u) {
    head = ((16u - (uint32_t)((uintptr_t)src.S & 15u)) & 15u) / kSize;
    head = head < n ? head : n;
    const size_t groups = (n - head) / V;
    body_end = head + groups * V;
    const uint4* __restrict__ S16 = reinterpret_cast<const uint4*>(src.S + head);
    const uint32_t lane = threadIdx.x & 63u;
    const size_t wave = ((size_t)blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (size_t)gridDim.x * 4;
    // (the bounds are the wave's: every lane takes part in the shuffles)
    for (size_t g0 = wave * 64; g0 < groups; g0 += nwaves * 64) {
      const uint4 q = g0 + lane < groups ? S16[g0 + lane] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
      for (uint32_t k = 0; k < V; ++k) {
        const uint32_t j = k * 64u + lane, from = j / V, byte = (j % V) * kSize;
        const uint32_t w0 = __shfl(q.x, from), w1 = __shfl(q.y, from), w2 = __shfl(q.z, from), w3 = __shfl(q.w, from);
        const uint32_t w = byte < 4u ? w0 : byte < 8u ? w1 : byte < 12u ? w2 : w3;
        const T v = (T)(w >> ((byte & 3u) * 8u));
        const size_t i = head + g0 * V + j;
        if (i < body_end) take(i, (float)v);
      }
    }
  }
  const size_t rest = head + (n - body_end);
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < rest; e += (size_t)gridDim.x * 256) {
    const size_t i = e < head ? e : body_end + (e - head);
    take(i, (float)src.S[i]);
  }
  if (!kStore) commit_in_table_lds(ds, as, out);
}

// The gradient source's two dense passes (kStore: emit above).  The hand-round of k_classified
// does not carry a stencil, so the field is walked by coordinates: gradient_walk (cvr_gradient.h)
// hands every voxel's value and gradient magnitude to the lambda, and a lane inside the row
// classifies and emits its voxel.  A wave's stores of a step are 64 consecutive voxels.
template <class T, bool kStore>
__global__ __launch_bounds__(256) void k_gradient(GradientSrc<T> src, uint32_t format, void* __restrict__ density,
                                                  void* __restrict__ albedo, MedScan* __restrict__ out) {
  src.stage();
  float d0;
  float4 a0;
  src.voxel(0u, 0u, 0u, 0, d0, a0);
  DensityScan ds;
  AlbedoScan as(a0);
  const uint32_t nx = src.res[0], ny = src.res[1];
  gradient_walk(src.S, nx, ny, src.res[2], src.p.axes,
                [&](bool in, uint32_t x, uint32_t y, uint32_t z, float cur, float mag) {
                  if (!in) return;
                  float d;
                  float4 a;
                  src.classified(cur, mag, d, a);
                  emit<kStore>(((size_t)z * ny + y) * nx + x, d, a, format, ds, as, density, albedo);
                });
  if (!kStore) commit_in_table_lds(ds, as, out);
}

// ------------------------------------------------- clipped dense passes ---
// The dense passes of a clipped build (Clipped above).  They index the grid linearly, so a voxel's
// coordinates come from its index: a dense grid has fewer than 2^32 voxels, and i / nx and
// (i / nx) / ny are divisions of a u32 by launch constants, one multiply-high and two shifts each
// (fastdiv, cvr_walk.h), with no 64-bit and no hardware divide.  A wave's run of consecutive
// voxels is first judged whole, from the rows of its first and last voxel: when every row of the
// run lies outside the crop box in z or in y, the wave loads nothing (the decision is the wave's:
// one scalar branch) and a store pass writes the clipped voxel to each.
struct LinearGrid {
  uint32_t nx, ny;
  FastDiv dx, dy;
  __device__ __forceinline__ void coords(uint32_t i, uint32_t& x, uint32_t& y, uint32_t& z) const {
    const uint32_t row = fastdiv(i, dx);
    x = i - row * nx;
    z = fastdiv(row, dy);
    y = row - z * ny;
  }
  // voxels i0..i1 (i0 <= i1, a wave's run) lie in rows that the crop box excludes
  __device__ __forceinline__ bool rows_outside(const ClipRegion& r, uint32_t i0, uint32_t i1) const {
    const uint32_t r0 = fastdiv(i0, dx), r1 = fastdiv(i1, dx), z0 = fastdiv(r0, dy), z1 = fastdiv(r1, dy);
    bool out = z1 < r.lo[2] || z0 >= r.hi[2];
    if (z0 == z1) out = out || r1 - z0 * ny < r.lo[1] || r0 - z0 * ny >= r.hi[1];
    return __builtin_amdgcn_readfirstlane((int)out) != 0;
  }
};

// What a clipped dense pass does with voxel i, not in a skipped run: its coordinates, the test,
// the source's value through load() if it is kept, and emit.  Returns whether it is kept.
template <bool kStore, class Src, class Load>
__device__ __forceinline__ bool emit_clipped(const Src& src, const LinearGrid& g, size_t i, Load&& load, uint32_t format,
                                             DensityScan& ds, AlbedoScan& as, void* __restrict__ density,
                                             void* __restrict__ albedo) {
  uint32_t x, y, z;
  g.coords((uint32_t)i, x, y, z);
  float d = 0.0f;
  float4 a = src.a0;
  const bool keep = src.keeps(x, y, z);
  if (keep) load(d, a);
  emit<kStore>(i, d, a, format, ds, as, density, albedo);
  return keep;
}

// k_classified behind a clip: the same head, 16-byte groups and tail, the same hand-round.  The
// scan (kStore false) leaves a skipped run alone: a clipped voxel is (0, a0), which no result of
// the scans depends on, but for a0's own binary16 overflow, taken once at voxel 0.  The store adds
// the kept voxels to out->kept.
template <class T, bool kStore>
__global__ __launch_bounds__(256) void k_classified_clip(Clipped<ScalarSrc<T>> src, size_t n, LinearGrid g,
                                                         uint32_t format, void* __restrict__ density,
                                                         void* __restrict__ albedo, MedScan* __restrict__ out) {
  src.stage();
  DensityScan ds;
  AlbedoScan as(src.a0);
  uint32_t kept = 0;
  if (!kStore && blockIdx.x == 0 && threadIdx.x == 0) as.take(src.a0, 0, format);
  // (scalar(): the voxel's scalar, asked for only when the voxel is kept)
  auto take = [&](size_t i, auto&& scalar) {
    kept += emit_clipped<kStore>(
        src, g, i, [&](float& d, float4& a) { src.s.classified(scalar(), d, a); }, format, ds, as, density, albedo);
  };
  constexpr uint32_t kSize = (uint32_t)sizeof(T), V = kSize < 4u ? 16u / kSize : 1u;
  size_t head = 0, body_end = 0;
  if constexpr (V > 1u) {
    head = ((16u - (uint32_t)((uintptr_t)src.s.S & 15u)) & 15u) / kSize;
    head = head < n ? head : n;
    const size_t groups = (n - head) / V;
    body_end = head + groups * V;
    const uint4* __restrict__ S16 = reinterpret_cast<const uint4*>(src.s.S + head);
    const uint32_t lane = threadIdx.x & 63u;
    const size_t wave = ((size_t)blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (size_t)gridDim.x * 4;
    // (the bounds are the wave's: every lane takes part in the shuffles)
    for (size_t g0 = wave * 64; g0 < groups; g0 += nwaves * 64) {
      const size_t first = head + g0 * V, last = (first + 64u * V < body_end ? first + 64u * V : body_end) - 1u;
      const bool skip = g.rows_outside(src.r, (uint32_t)first, (uint32_t)last);
      if (!kStore && skip) continue;
      const uint4 q = !skip && g0 + lane < groups ? S16[g0 + lane] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
      for (uint32_t k = 0; k < V; ++k) {
        const uint32_t j = k * 64u + lane, from = j / V, byte = (j % V) * kSize;
        const uint32_t w0 = __shfl(q.x, from), w1 = __shfl(q.y, from), w2 = __shfl(q.z, from), w3 = __shfl(q.w, from);
        const uint32_t w = byte < 4u ? w0 : byte < 8u ? w1 : byte < 12u ? w2 : w3;
        const T v = (T)(w >> ((byte & 3u) * 8u));
        const size_t i = first + j;
        if (i < body_end) take(i, [&] { return (float)v; });
      }
    }
  }
  const size_t rest = head + (n - body_end);
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < rest; e += (size_t)gridDim.x * 256) {
    const size_t i = e < head ? e : body_end + (e - head);
    take(i, [&] { return (float)src.s.S[i]; });
  }
  if (!kStore)
    commit_in_table_lds(ds, as, out);
  else
    commit_kept(kept, out);
}

// k_gradient behind a clip: the walk reads the field as it does without one (a kept voxel's
// stencil needs its clipped neighbours), and a lane tests its voxel before it classifies it.  A
// task whose box (256 x of one row over 16 planes) is provably clipped is not walked: the
// workgroup's decision; the store writes the clipped voxel to each of its voxels, the scan has
// nothing to take of them but a0's own overflow, taken once at voxel 0.
template <class T, bool kStore>
__global__ __launch_bounds__(256) void k_gradient_clip(Clipped<GradientSrc<T>> src, uint32_t format,
                                                       void* __restrict__ density, void* __restrict__ albedo,
                                                       MedScan* __restrict__ out) {
  src.stage();
  DensityScan ds;
  AlbedoScan as(src.a0);
  uint32_t kept = 0;
  const uint32_t nx = src.s.res[0], ny = src.s.res[1];
  if (!kStore && blockIdx.x == 0 && threadIdx.x == 0) as.take(src.a0, 0, format);
  gradient_walk(
      src.s.S, nx, ny, src.s.res[2], src.s.p.axes,
      [&](bool in, uint32_t x, uint32_t y, uint32_t z, float cur, float mag) {
        if (!in) return;
        float d = 0.0f;
        float4 a = src.a0;
        if (src.keeps(x, y, z)) {
          src.s.classified(cur, mag, d, a);
          ++kept;
        }
        emit<kStore>(((size_t)z * ny + y) * nx + x, d, a, format, ds, as, density, albedo);
      },
      [&](uint32_t xb, uint32_t x, uint32_t y, uint32_t z0, uint32_t z1) {
        const uint32_t xe = xb + 255u;
        const uint32_t e0[3] = {xb, y, z0}, e1[3] = {xe < nx ? xe : nx - 1u, y, z1 - 1u};
        if (!clip_box_outside(src.r, e0, e1)) return false;
        if (kStore && x < nx)
          for (uint32_t z = z0; z < z1; ++z)
            emit<true>(((size_t)z * ny + y) * nx + x, 0.0f, src.a0, format, ds, as, density, albedo);
        return true;
      });
  if (!kStore)
    commit_in_table_lds(ds, as, out);
  else
    commit_kept(kept, out);
}

// The arrays' source behind a clip, dense: one voxel per lane, a wave's run 64 consecutive voxels
// (256 bytes of density, 1 KiB of albedo per load).  kStore false: k_scan_density's and, with an
// albedo array, k_scan_albedo's results of the clipped values, together.  kStore true: the voxels
// into the context's density grid and, with an albedo array, its albedo grid (format 1: as
// binary16), and the kept voxels into out->kept.
template <bool kStore>
__global__ __launch_bounds__(256) void k_arrays_clip(Clipped<ArraySrc> src, size_t n, LinearGrid g, uint32_t format,
                                                     void* __restrict__ density, void* __restrict__ albedo,
                                                     MedScan* __restrict__ out) {
  src.stage();
  const bool with_albedo = src.has_albedo();
  DensityScan ds;
  AlbedoScan as(src.a0);
  uint32_t kept = 0;
  if (!kStore && with_albedo && blockIdx.x == 0 && threadIdx.x == 0) as.take(src.a0, 0, format);
  // (the bounds are the workgroup's; a wave past the end has no voxel)
  for (size_t base = (size_t)blockIdx.x * 256; base < n; base += (size_t)gridDim.x * 256) {
    const size_t i0 = base + (threadIdx.x & ~63u), i = base + threadIdx.x;
    if (i0 >= n) continue;
    const bool skip = g.rows_outside(src.r, (uint32_t)i0, (uint32_t)(i0 + 63u < n ? i0 + 63u : n - 1u));
    if (!kStore && skip) continue;
    if (i >= n) continue;
    uint32_t x, y, z;
    g.coords((uint32_t)i, x, y, z);
    float d = 0.0f;
    float4 a = src.a0;
    if (!skip) {
      src.s.voxel(i, d, a);
      const bool keep = src.keeps(x, y, z);
      d = keep ? d : 0.0f;
      a = keep_or(keep, a, src.a0);
      kept += keep;
    }
    if (!kStore) {
      ds.take(d, i, format);
      if (with_albedo) as.take(a, i, format);
    } else if (format) {
      reinterpret_cast<_Float16*>(density)[i] = (_Float16)d;
      if (with_albedo) reinterpret_cast<uint2*>(albedo)[i] = half4_bits(a);
    } else {
      reinterpret_cast<float*>(density)[i] = d;
      if (with_albedo) reinterpret_cast<float4*>(albedo)[i] = a;
    }
  }
  __shared__ float s_mx[4];
  __shared__ unsigned long long s_ov[8];
  __shared__ uint32_t s_fl[4];
  if (!kStore) {
    ds.commit(s_mx, s_ov, out);
    as.commit(s_fl, s_ov + 4, out);
  } else {
    commit_kept(kept, out);
  }
}

// 1: the labels of the 16-byte groups are loaded wide and brought into place by a byte funnel;
// 0: one label byte per lane and step (the A/B partner, profiles/labels/README.md)
#ifndef CVR_LABEL_WIDE
#define CVR_LABEL_WIDE 1
#endif
typedef uint32_t label_words4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t label_words2 __attribute__((ext_vector_type(2), aligned(4)));

// The labelled source's two dense passes, with or without a clip (Src: LabeledSrc<T> or
// Clipped<LabeledSrc<T>>; kStore: emit above).  k_classified's streaming shape: an integer field
// is cut into a head up to its first 16-byte boundary, whole 16-byte groups and a tail; a wave
// loads 64 groups and hands the voxels round so that in step k lane l has voxel 64 k + l of its
// run.  The labels of the same voxels come along as a second stream.  A lane's group of V voxels
// has V label bytes, at an address whose alignment has nothing to do with the field's: the lane
// loads the V / 4 aligned words that cover them and, when the bytes do not start on a word, the
// word after (an aligned word that holds a byte of the volume lies in the volume's page), and a
// byte funnel (v_alignbyte_b32) shifts them into place, by the one offset r = address & 3 of the
// whole launch.  The label words are then handed round by the shuffles that hand the scalars round.
// Of the two ways to an unaligned second stream, this and a hand-round of the labels' own from
// word-per-lane loads, the funnel was built and measured against a byte per lane and step
// (CVR_LABEL_WIDE 0; profiles/labels/README.md has the figures); the second hand-round was not built.
// Head and tail (a float field: every voxel) take one voxel and one label byte per lane, a wave's
// lanes consecutive voxels.  Behind a clip a wave's run that lies in rows outside the crop box is
// not read (LinearGrid::rows_outside), as in k_classified_clip.  The store counts the kept voxels
// per label byte (LabelCounts) and, behind a clip, the kept voxels.
template <class Src, bool kStore>
__global__ __launch_bounds__(256) void k_labeled(Src src, size_t n, LinearGrid g, uint32_t format,
                                                 void* __restrict__ density, void* __restrict__ albedo,
                                                 MedScan* __restrict__ out) {
  constexpr bool kClip = is_clipped<Src>::value;
  using T = typename Src::Scalar;
  const LabeledSrc<T>& ls = labeled(src);
  [[maybe_unused]] LabelCounts lc;
  if constexpr (kStore) lc.begin();
  src.stage();
  float4 a0;
  if constexpr (kClip) {
    a0 = src.a0;
  } else {
    float d0;
    ls.voxel(0, d0, a0);
  }
  DensityScan ds;
  AlbedoScan as(a0);
  [[maybe_unused]] uint32_t kept = 0;
  if constexpr (kClip) {
    if (!kStore && blockIdx.x == 0 && threadIdx.x == 0) as.take(a0, 0, format);
  }
  // voxel i with scalar s and label byte label, in the lanes that have one (every lane of the
  // wave calls this: the counters' merge is the wave's)
  auto take = [&](size_t i, bool has, float s, uint32_t label) {
    bool keep = has;
    if (has) {
      float d = 0.0f;
      float4 a = a0;
      if constexpr (kClip) {
        uint32_t x, y, z;
        g.coords((uint32_t)i, x, y, z);
        keep = src.keeps(x, y, z);
      }
      if (keep) ls.classified(s, label, d, a);
      emit<kStore>(i, d, a, format, ds, as, density, albedo);
    }
    if constexpr (kStore) lc.add(label, keep);
    if constexpr (kClip) kept += keep;
  };
  constexpr uint32_t kSize = (uint32_t)sizeof(T), V = kSize < 4u ? 16u / kSize : 1u;
  const uint32_t lane = threadIdx.x & 63u;
  size_t head = 0, body_end = 0;
  if constexpr (V > 1u) {
    constexpr uint32_t W = V / 4u;  // label words of a group
    head = ((16u - (uint32_t)((uintptr_t)ls.S & 15u)) & 15u) / kSize;
    head = head < n ? head : n;
    const size_t groups = (n - head) / V;
    body_end = head + groups * V;
    const uint4* __restrict__ S16 = reinterpret_cast<const uint4*>(ls.S + head);
    const uintptr_t la = (uintptr_t)(ls.L + head);
    [[maybe_unused]] const uint32_t r = (uint32_t)(la & 3u);
    [[maybe_unused]] const uint32_t* __restrict__ Lw = reinterpret_cast<const uint32_t*>(la - r);
    const size_t wave = ((size_t)blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (size_t)gridDim.x * 4;
    // (the bounds are the wave's: every lane takes part in the shuffles)
    for (size_t g0 = wave * 64; g0 < groups; g0 += nwaves * 64) {
      const size_t first = head + g0 * V;
      if constexpr (kClip) {
        const size_t last = (first + 64u * V < body_end ? first + 64u * V : body_end) - 1u;
        if (g.rows_outside(src.r, (uint32_t)first, (uint32_t)last)) {
          if constexpr (kStore) {
#pragma unroll
            for (uint32_t k = 0; k < V; ++k) {
              const size_t i = first + k * 64u + lane;
              if (i < body_end) emit<true>(i, 0.0f, a0, format, ds, as, density, albedo);
            }
          }
          continue;
        }
      }
      const bool have = g0 + lane < groups;
      const uint4 q = have ? S16[g0 + lane] : make_uint4(0u, 0u, 0u, 0u);
      uint32_t lb[W];
#if CVR_LABEL_WIDE
      uint32_t lw[W + 1u];
#pragma unroll
      for (uint32_t c = 0; c <= W; ++c) lw[c] = 0u;
      if (have) {
        const uint32_t* __restrict__ w = Lw + (g0 + lane) * W;
        if constexpr (W == 4u) {
          const label_words4 t = *reinterpret_cast<const label_words4*>(w);
          lw[0] = t.x, lw[1] = t.y, lw[2] = t.z, lw[3] = t.w;
        } else {
          const label_words2 t = *reinterpret_cast<const label_words2*>(w);
          lw[0] = t.x, lw[1] = t.y;
        }
        if (r) lw[W] = w[W];
      }
#pragma unroll
      for (uint32_t c = 0; c < W; ++c) lb[c] = __builtin_amdgcn_alignbyte(lw[c + 1u], lw[c], r);
#endif
#pragma unroll
      for (uint32_t k = 0; k < V; ++k) {
        const uint32_t j = k * 64u + lane, from = j / V, e = j % V, byte = e * kSize;
        const uint32_t w0 = __shfl(q.x, from), w1 = __shfl(q.y, from), w2 = __shfl(q.z, from), w3 = __shfl(q.w, from);
        const uint32_t w = byte < 4u ? w0 : byte < 8u ? w1 : byte < 12u ? w2 : w3;
        const T v = (T)(w >> ((byte & 3u) * 8u));
        const size_t i = first + j;
        const bool has = i < body_end;
        uint32_t label;
#if CVR_LABEL_WIDE
        uint32_t lx = __shfl(lb[0], from);
#pragma unroll
        for (uint32_t c = 1; c < W; ++c) {
          const uint32_t t = __shfl(lb[c], from);
          lx = (e >> 2) == c ? t : lx;
        }
        label = (lx >> ((e & 3u) * 8u)) & 0xFFu;
#else
        (void)lb;
        label = has ? ls.L[i] : 0u;
#endif
        take(i, has, (float)v, label);
      }
    }
  }
  const size_t rest = head + (n - body_end);
  // (the bounds are the wave's here too)
  for (size_t e0 = (size_t)blockIdx.x * 256 + (threadIdx.x & ~63u); e0 < rest; e0 += (size_t)gridDim.x * 256) {
    const size_t e = e0 + lane;
    const bool has = e < rest;
    const size_t i = e < head ? e : body_end + (e - head);
    if constexpr (kClip && V == 1u) {
      // a float field: the wave's 64 consecutive voxels
      if (g.rows_outside(src.r, (uint32_t)e0, (uint32_t)(e0 + 63u < n ? e0 + 63u : n - 1u))) {
        if (kStore && has) emit<true>(i, 0.0f, a0, format, ds, as, density, albedo);
        continue;
      }
    }
    float s = 0.0f;
    uint32_t label = 0u;
    if (has) {
      s = (float)ls.S[i];
      label = ls.L[i];
    }
    take(i, has, s, label);
  }
  if constexpr (!kStore) {
    commit_in_table_lds(ds, as, out);
  } else {
    lc.flush(ls.counts);
    if constexpr (kClip) commit_kept(kept, out);
  }
}

// The context's albedo grid filled with one value (CVR_DEVMED_CONST_ALBEDO, dense).
__global__ __launch_bounds__(256) void k_fill_albedo(void* __restrict__ dst, size_t n, uint32_t format, float4 v) {
  const uint2 h = half4_bits(v);
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
// A classified source reads one scalar per lane and row here (a wave's run is 64 to 256 bytes),
// always looks at the colours, and finds the value scans' results on the way (scan), so that a
// sparse build reads the field once here and once in the gather.  A labelled source also counts
// the kept voxels per label byte here (LabelCounts), the pass that sees every in-grid voxel once.
template <class Src>
__global__ __launch_bounds__(256) void k_leaf_flags(Src src, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t lnx,
                                                    uint32_t lny, uint32_t lnz, uint32_t* __restrict__ flags,
                                                    uint32_t format, MedScan* __restrict__ scan) {
  constexpr bool kScan = !std::is_void_v<typename Src::Scalar>, kClip = is_clipped<Src>::value;
  constexpr bool kLabels = is_labeled<Src>::value;
  [[maybe_unused]] LabelCounts lc;
  if constexpr (kLabels) lc.begin();
  src.stage();
  const uint32_t nxc = (lnx + kLeafRunLeaves - 1u) / kLeafRunLeaves;
  const size_t ntasks = (size_t)nxc * lny * lnz;
  const bool with_albedo = src.has_albedo();
  uint32_t b0 = 0, b1 = 0, b2 = 0, b3 = 0;
  if (with_albedo) {
    float d;
    float4 f;
    src.voxel(0u, 0u, 0u, 0, d, f);
    b0 = __float_as_uint(f.x), b1 = __float_as_uint(f.y), b2 = __float_as_uint(f.z), b3 = __float_as_uint(f.w);
  }
  DensityScan ds;
  AlbedoScan as(make_float4(__uint_as_float(b0), __uint_as_float(b1), __uint_as_float(b2), __uint_as_float(b3)));
  [[maybe_unused]] uint32_t kept = 0;
  if constexpr (kClip && kScan) {
    // voxel 0's albedo is a0 kept or clipped, and a skipped task is not scanned: its binary16
    // overflow, the smallest index there can be, is taken here
    if (blockIdx.x == 0 && threadIdx.x == 0) as.take(src.a0, 0, format);
  }
  for (size_t t = blockIdx.x; t < ntasks; t += gridDim.x) {
    const uint32_t xc = (uint32_t)(t % nxc), ly = (uint32_t)((t / nxc) % lny), lz = (uint32_t)(t / ((size_t)nxc * lny));
    const uint32_t x = xc * kLeafRunVoxels + threadIdx.x;
    uint32_t any = 0;
    bool read = x < nx;
    if constexpr (kClip) {
      // the task's in-grid extent, wholly clipped by its box test (the workgroup's decision): no
      // leaf of it exists, and the field is not read
      const uint32_t xe = xc * kLeafRunVoxels + kLeafRunVoxels - 1u;
      const uint32_t e0[3] = {xc * kLeafRunVoxels, ly * 8u, lz * 8u};
      const uint32_t e1[3] = {xe < nx ? xe : nx - 1u, ly * 8u + 7u < ny ? ly * 8u + 7u : ny - 1u,
                              lz * 8u + 7u < nz ? lz * 8u + 7u : nz - 1u};
      read = read && !clip_box_outside(src.r, e0, e1);
    }
    if (read) {
#pragma unroll 8
      for (uint32_t r = 0; r < 64u; ++r) {
        const uint32_t y = ly * 8u + (r & 7u), z = lz * 8u + (r >> 3);
        if (y < ny && z < nz) {
          const size_t i = ((size_t)z * ny + y) * nx + x;
          float d;
          float4 a;
          if constexpr (kClip) {
            const bool keep = src.voxel(x, y, z, i, d, a);
            kept += keep;
            if constexpr (kLabels) lc.add(labeled(src).L[i], keep);
          } else {
            src.voxel(x, y, z, i, d, a);
            if constexpr (kLabels) lc.add(labeled(src).L[i], true);
          }
          if (kScan) {
            ds.take(d, i, format);
            as.take(a, i, format);
          }
          any |= d != 0.0f;
          if (with_albedo)
            any |= __float_as_uint(a.x) != b0 || __float_as_uint(a.y) != b1 || __float_as_uint(a.z) != b2 ||
                   __float_as_uint(a.w) != b3;
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
  if constexpr (kScan) commit_in_table_lds(ds, as, scan);
  if constexpr (kClip) commit_kept(kept, scan);
  if constexpr (kLabels) lc.flush(labeled(src).counts);
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
__global__ __launch_bounds__(kScanSumsChunk) void k_scan_sums(uint32_t* __restrict__ sums, uint32_t nb,
                                                    uint32_t* __restrict__ total) {
  __shared__ uint32_t s_w[16];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < nb; base += kScanSumsChunk) {
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
template <class Src, bool kStore>
__global__ __launch_bounds__(256) void k_gather_leaves(Src src, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t lnx,
                                                       uint32_t lny, const uint32_t* __restrict__ slot_leaf,
                                                       size_t n_pool, float4 bg, uint32_t format,
                                                       void* __restrict__ leaf_density, void* __restrict__ leaf_albedo,
                                                       MedScan* __restrict__ out) {
  src.stage();
  const bool with_albedo = src.has_albedo();
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n_pool; p += (size_t)gridDim.x * 256) {
    const uint32_t leaf = slot_leaf[p >> 9], local = (uint32_t)p & 511u;
    const uint32_t lx = leaf % lnx, ly = (leaf / lnx) % lny, lz = leaf / (lnx * lny);
    const uint32_t x = lx * 8u + (local & 7u), y = ly * 8u + ((local >> 3) & 7u), z = lz * 8u + (local >> 6);
    bool in = x < nx && y < ny && z < nz;
    if constexpr (is_clipped<Src>::value) {
      // A wave's 64 pool voxels are one 8 x 8 slice (one z) of one leaf.  The slice's in-grid box
      // is judged by the box test (outside the crop, or its corners on one plane's negative side:
      // the wave's decision), and a clipped slice is written as (0, bg) unread.  bg is a0: the
      // clipped voxel's albedo and the out-of-grid voxel's are the same 16 bytes.  (The leaf's
      // whole box is not asked: a stored leaf has a kept voxel.)
      if (z < nz) {
        const uint32_t x0 = lx * 8u, y0 = ly * 8u;
        const uint32_t e0[3] = {x0, y0, z}, e1[3] = {x0 + 7u < nx ? x0 + 7u : nx - 1u, y0 + 7u < ny ? y0 + 7u : ny - 1u, z};
        in = in && !clip_box_outside(src.r, e0, e1);
      }
    }
    float d = 0.0f;
    float4 a = bg;
    if (in) src.voxel(x, y, z, ((size_t)z * ny + y) * nx + x, d, a);
    if (kStore) {
      if (format)
        reinterpret_cast<_Float16*>(leaf_density)[p] = (_Float16)d;
      else
        reinterpret_cast<float*>(leaf_density)[p] = d;
    } else if (half_overflow(d)) {
      atomicMin(&out->ovf_density, (unsigned long long)p);
    }
    if (with_albedo) {
      if (!kStore) {
        const unsigned long long at =
            half_overflow(a.x) ? 4 * p : half_overflow(a.y) ? 4 * p + 1 : half_overflow(a.z) ? 4 * p + 2 : kNoIndex;
        if (at != kNoIndex) atomicMin(&out->ovf_albedo, at);
      } else if (format) {
        reinterpret_cast<uint2*>(leaf_albedo)[p] = half4_bits(a);
      } else {
        reinterpret_cast<float4*>(leaf_albedo)[p] = a;
      }
    }
  }
}

uint32_t stream_grid(size_t n) { return (uint32_t)std::min<size_t>((n + 255) / 256, kStreamGridCap); }
// the scans: 8 resident workgroups per CU of 256, each looping
uint32_t scan_grid(size_t n) { return (uint32_t)std::min<size_t>((n + 255) / 256, kScanGridCap); }

// f(src, lds): the source as the kernels take it and the dynamic LDS its table needs
template <class F>
void with_source(const VoxelSource& v, bool with_albedo, F f) {
  // (the classified scan's reduction reuses the table's LDS: at least 8 entries)
  const size_t lds =
      (size_t)std::max(v.gradient ? v.gtf.n * v.gtf.m : v.labels ? v.tf.n * v.label_rows : v.tf.n, 8u) * sizeof(float4);
  const uint32_t al = with_albedo ? 1u : 0u;
  auto labeled_src = [&](auto* S) {
    using T = std::remove_cv_t<std::remove_pointer_t<decltype(S)>>;
    f(LabeledSrc<T>{S, v.labels, v.table, v.tf, v.label_rows, v.label_counts, al, nullptr}, lds);
  };
  auto gradient = [&](auto* S) {
    using T = std::remove_cv_t<std::remove_pointer_t<decltype(S)>>;
    f(GradientSrc<T>{S, v.table, v.gtf, {v.res[0], v.res[1], v.res[2]}, al, nullptr}, lds);
  };
  if (v.gradient && v.scalar_type == 1u)
    gradient(static_cast<const uint8_t*>(v.scalar));
  else if (v.gradient && v.scalar_type == 2u)
    gradient(static_cast<const uint16_t*>(v.scalar));
  else if (v.gradient && v.scalar_type == 3u)
    gradient(static_cast<const int16_t*>(v.scalar));
  else if (v.gradient)
    gradient(static_cast<const float*>(v.scalar));
  else if (v.labels && v.scalar_type == 1u)
    labeled_src(static_cast<const uint8_t*>(v.scalar));
  else if (v.labels && v.scalar_type == 2u)
    labeled_src(static_cast<const uint16_t*>(v.scalar));
  else if (v.labels && v.scalar_type == 3u)
    labeled_src(static_cast<const int16_t*>(v.scalar));
  else if (v.labels)
    labeled_src(static_cast<const float*>(v.scalar));
  else if (!v.scalar)
    f(ArraySrc{v.density, with_albedo ? reinterpret_cast<const float4*>(v.albedo) : nullptr}, (size_t)0);
  else if (v.scalar_type == 1u)
    f(ScalarSrc<uint8_t>{static_cast<const uint8_t*>(v.scalar), v.table, v.tf, al, nullptr}, lds);
  else if (v.scalar_type == 2u)
    f(ScalarSrc<uint16_t>{static_cast<const uint16_t*>(v.scalar), v.table, v.tf, al, nullptr}, lds);
  else if (v.scalar_type == 3u)
    f(ScalarSrc<int16_t>{static_cast<const int16_t*>(v.scalar), v.table, v.tf, al, nullptr}, lds);
  else
    f(ScalarSrc<float>{static_cast<const float*>(v.scalar), v.table, v.tf, al, nullptr}, lds);
}

float4 clip_a0(const VoxelSource& v) { return make_float4(v.clip_a0[0], v.clip_a0[1], v.clip_a0[2], v.clip_a0[3]); }
// The same, behind the source's clip region when it has one: f then gets a Clipped source, and
// the launch runs the kernel's clipped instance (a source without a clip runs today's)
template <class F>
void with_clipped_source(const VoxelSource& v, bool with_albedo, F f) {
  with_source(v, with_albedo, [&](auto src, size_t lds) {
    if (v.clip)
      f(Clipped<decltype(src)>{src, *v.clip, clip_a0(v)}, lds);
    else
      f(src, lds);
  });
}
LinearGrid linear_grid(const uint32_t res[3]) { return {res[0], res[1], make_fastdiv(res[0]), make_fastdiv(res[1])}; }

template <bool kStore>
hipError_t launch_classified(const VoxelSource& v, size_t n, uint32_t format, void* density, void* albedo,
                             MedScan* out, hipStream_t s) {
  if (!v.scalar) return hipErrorInvalidValue;
  with_clipped_source(v, true, [&](auto src, size_t lds) {
    using Src = decltype(src);
    using T = typename Src::Scalar;
    if constexpr (is_labeled<Src>::value) {
      hipLaunchKernelGGL((k_labeled<Src, kStore>), dim3(scan_grid(n)), dim3(256), lds, s, src, n, linear_grid(v.res),
                         format, density, albedo, out);
    } else if constexpr (std::is_same_v<Src, Clipped<ScalarSrc<T>>>) {
      hipLaunchKernelGGL((k_classified_clip<T, kStore>), dim3(scan_grid(n)), dim3(256), lds, s, src, n,
                         linear_grid(v.res), format, density, albedo, out);
    } else if constexpr (is_clipped<Src>::value && !std::is_void_v<T>) {
      const uint32_t grid = (uint32_t)std::min<size_t>(gradient_walk_tasks(v.res[0], v.res[1], v.res[2]), kWalkTaskCap);
      hipLaunchKernelGGL((k_gradient_clip<T, kStore>), dim3(grid >= 8u ? grid & ~7u : grid), dim3(256), lds, s,
                         src, format, density, albedo, out);
    } else if constexpr (std::is_same_v<Src, ScalarSrc<T>>) {
      hipLaunchKernelGGL((k_classified<T, kStore>), dim3(scan_grid(n)), dim3(256), lds, s, src, n, format, density,
                         albedo, out);
    } else if constexpr (!std::is_void_v<T>) {
      // (a multiple of 8 workgroups where there are 8: the walk's XCD turn needs one)
      const uint32_t grid = (uint32_t)std::min<size_t>(gradient_walk_tasks(v.res[0], v.res[1], v.res[2]), kWalkTaskCap);
      hipLaunchKernelGGL((k_gradient<T, kStore>), dim3(grid >= 8u ? grid & ~7u : grid), dim3(256), lds, s,
                         src, format, density, albedo, out);
    }
  });
  return hipGetLastError();
}

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

hipError_t launch_scan_classified(const VoxelSource& src, size_t n, uint32_t format, MedScan* out, hipStream_t s) {
  return launch_classified<false>(src, n, format, nullptr, nullptr, out, s);
}

hipError_t launch_store_classified(const VoxelSource& src, size_t n, uint32_t format, void* density, void* albedo,
                                   MedScan* scan, hipStream_t s) {
  return launch_classified<true>(src, n, format, density, albedo, scan, s);
}

hipError_t launch_scan_clipped(const VoxelSource& v, const uint32_t res[3], uint32_t format, MedScan* out,
                               hipStream_t s) {
  if (!v.clip || v.scalar) return hipErrorInvalidValue;
  const size_t n = (size_t)res[0] * res[1] * res[2];
  const Clipped<ArraySrc> src{{v.density, reinterpret_cast<const float4*>(v.albedo)}, *v.clip, clip_a0(v)};
  hipLaunchKernelGGL(k_arrays_clip<false>, dim3(scan_grid(n)), dim3(256), 0, s, src, n, linear_grid(res), format,
                     nullptr, nullptr, out);
  return hipGetLastError();
}

hipError_t launch_store_clipped(const VoxelSource& v, const uint32_t res[3], uint32_t format, void* density,
                                void* albedo, MedScan* scan, hipStream_t s) {
  if (!v.clip || v.scalar) return hipErrorInvalidValue;
  const size_t n = (size_t)res[0] * res[1] * res[2];
  const Clipped<ArraySrc> src{{v.density, reinterpret_cast<const float4*>(v.albedo)}, *v.clip, clip_a0(v)};
  hipLaunchKernelGGL(k_arrays_clip<true>, dim3(stream_grid(n)), dim3(256), 0, s, src, n, linear_grid(res), format,
                     density, albedo, scan);
  return hipGetLastError();
}

hipError_t launch_leaf_flags(const VoxelSource& v, bool with_albedo, const uint32_t res[3], const uint32_t ln[3],
                             uint32_t* flags, uint32_t format, MedScan* scan, hipStream_t s) {
  const size_t ntasks = (size_t)((ln[0] + kLeafRunLeaves - 1u) / kLeafRunLeaves) * ln[1] * ln[2];
  with_clipped_source(v, with_albedo, [&](auto src, size_t lds) {
    hipLaunchKernelGGL(k_leaf_flags<decltype(src)>, dim3((uint32_t)std::min<size_t>(ntasks, kLeafFlagsGridCap)),
                       dim3(256), lds, s, src, res[0], res[1], res[2], ln[0], ln[1], ln[2], flags, format, scan);
  });
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
  hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(kScanSumsChunk), 0, s, sums, nb, total);
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

hipError_t launch_gather_leaves(const VoxelSource& v, bool with_albedo, const uint32_t res[3], const uint32_t ln[3],
                                const uint32_t* slot_leaf, size_t n_leaves, const float bg[4], uint32_t format,
                                void* leaf_density, void* leaf_albedo, MedScan* check, hipStream_t s) {
  const size_t np = n_leaves * 512;
  if (np == 0) return hipSuccess;
  const float4 b = make_float4(bg[0], bg[1], bg[2], bg[3]);
  with_clipped_source(v, with_albedo, [&](auto src, size_t lds) {
    using Src = decltype(src);
    if (check)
      hipLaunchKernelGGL((k_gather_leaves<Src, false>), dim3(stream_grid(np)), dim3(256), lds, s, src, res[0], res[1],
                         res[2], ln[0], ln[1], slot_leaf, np, b, format, nullptr, nullptr, check);
    else
      hipLaunchKernelGGL((k_gather_leaves<Src, true>), dim3(stream_grid(np)), dim3(256), lds, s, src, res[0], res[1],
                         res[2], ln[0], ln[1], slot_leaf, np, b, format, leaf_density, leaf_albedo, nullptr);
  });
  return hipGetLastError();
}

}  // namespace cvr
