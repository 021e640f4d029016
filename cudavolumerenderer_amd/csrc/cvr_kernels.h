// cvr_kernels.h - host-side launch entry points of cvr_kernels.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cvr_clip.h"
#include "cvr_env.h"
#include "cvr_gradient.h"
#include "cvr_walk.h"
#include "cvr_wpool_select.h"

namespace cvr {

// Per-context work area (cvr_ctx d_work, zeroed per launch: cvr_launch.cpp), in bytes:
// 16 u64 stats at 0, 16 u64 diagnostic counters at 128, up to 64 queue heads
// from 256 (one 64-byte line each, LaunchParams::queue).
constexpr size_t kWorkStats = 0, kWorkDebug = 128, kWorkQueues = 256, kMaxQueues = 64;
constexpr size_t kWorkBytesBase = kWorkQueues + kMaxQueues * 64;

// Per-path debug record; layout identical to cvr_path_record (include/cvr.h)
// and oracle_path (oracle/cvr_oracle.c).
struct PathRecord {
  uint32_t image_id;
  uint32_t flags;  // bit0 escaped (contributed), bit1 truncated
  float T[3];
  uint32_t n_segments, n_steps, n_density, n_albedo;
};

// Ray-slot pool of the wavefront scheduler (cvr_wavefront.hip), SoA in HBM.
struct WfPool {
  float *ox, *oy, *oz, *dx, *dy, *dz, *tx, *ty, *tz, *dist, *t;
  uint32_t *r0, *r1, *r2, *r3, *r4, *rd;
  uint32_t* img;
  uint32_t* meta;    // state | normal code << 2 | segments << 8
  uint32_t* cursor;  // per events-wave [q_next, q_end) into the path-id range
  unsigned int* head;  // global path-id dequeue head
  unsigned int* alive; // set by the events kernel when a slot needs tracking
  unsigned long long* stats_events;  // per events-wave rows of 8 counters
  unsigned long long* stats_track;   // per track-wave rows of 8 counters
  uint32_t n;        // slots
};

hipError_t wf_launch_events(const MediumParams& m, const LaunchParams& L, const WfPool& P, bool scatter_eps,
                            hipStream_t s);
hipError_t wf_launch_track(const MediumParams& m, const LaunchParams& L, const WfPool& P, uint32_t grid,
                           hipStream_t s);
hipError_t wf_track_occupancy(int* blocks_per_cu);
hipError_t wf_launch_reduce(const unsigned long long* rows, uint32_t nrows, unsigned long long* out, hipStream_t s);

hipError_t launch_naive(const MediumParams& m, const LaunchParams& L, bool scatter_eps, hipStream_t s);
hipError_t launch_persistent(const MediumParams& m, const LaunchParams& L, bool scatter_eps, int waves,
                             uint32_t grid, hipStream_t s);
hipError_t persistent_occupancy(bool scatter_eps, int waves, int* blocks_per_cu);
hipError_t launch_trace(const MediumParams& m, const LaunchParams& L, bool scatter_eps, PathRecord* rec,
                        hipStream_t s);
// cvr_trace_env: launch_trace's walk with the environment applied at the escape; layout identical to
// cvr_env_record (include/cvr.h).  env: the map's header in device memory.
struct EnvRecord {
  uint32_t image_id, flags, n_segments;
  float T[3], d[3], C[3];
};
hipError_t launch_trace_env(const MediumParams& m, const LaunchParams& L, bool scatter_eps, const EnvParams* env,
                            EnvRecord* rec, hipStream_t s);
hipError_t launch_pool(const MediumParams& m, const LaunchParams& L, bool scatter_eps, uint32_t grid, hipStream_t s);
hipError_t pool_occupancy(bool scatter_eps, int* blocks_per_cu);
// The wave pool: the instance wpool_select (cvr_wpool_select.h) gives for request q, which the
// caller fills to describe m and L (q.moments: L.out holds 2 * tile_px float4, the moments behind
// the tile).  hipErrorInvalidValue: no instance runs q, or grid is not whole workgroups.
hipError_t launch_wpool(const MediumParams& m, const LaunchParams& L, const WpoolRequest& q, uint32_t grid,
                        hipStream_t s);
// The three below take an instance that wpool_select returned.
// Resident waves per CU of the wave-pool instance (workgroups per CU x waves per workgroup).
hipError_t wpool_occupancy(const WpoolInstance& k, int* waves_per_cu);
// Pool slots per wave of the wave-pool kernel instance (LaunchParams::pool_T
// needs grid * slots float4).
uint32_t wpool_slots(const WpoolInstance& k);
// Waves per workgroup of the wave-pool instance: 1 for dense media; sparse media run
// several wave-private pools per workgroup that share one LDS copy of the launch
// parameters and the empty-region mask.  A wave-pool grid (in waves) is a multiple.
uint32_t wpool_wpg(const WpoolInstance& k);
// The instances the library ships, in table order (cvr_debug_wpool_rows; host only, no device): at most
// `capacity` of them are written to out (which may be null when capacity is 0); returns their number.
uint32_t wpool_rows(WpoolInstance* out, uint32_t capacity);
// regenerationSK with the RNG bound to the persistent thread (CVR_OPT_RNG_BINDING 1):
// `grid` one-wave workgroups, path ids from the launch's single queue head.
hipError_t launch_regen_thread(const MediumParams& m, const LaunchParams& L, bool scatter_eps, uint32_t grid,
                               hipStream_t s);
// streamingSK / sortingSK with the thread-bound RNG (CVR_OPT_RNG_BINDING 1): blocks of 256 threads
hipError_t launch_stream_thread(const MediumParams& m, const LaunchParams& L, bool sorting, uint32_t grid,
                                hipStream_t s);
// streamingMK with the thread-bound RNG (CVR_OPT_RNG_BINDING 1): the reference's regenerate /
// extend pair per iteration of a host loop, 256-thread blocks, one slot per thread.
struct SmkSlots {
  float4* a;     // (o, image_id bits)
  float4* b;     // (d, segments bits)
  float4* t;     // (T, 0)
  uint8_t* act;  // path active
};
hipError_t launch_smk_regen(const LaunchParams& L, const SmkSlots& out, uint4* st0, uint2* st1, uint32_t* ctl,
                            uint32_t grid, hipStream_t s);
hipError_t launch_smk_extend(const MediumParams& m, const LaunchParams& L, const SmkSlots& in, const SmkSlots& out,
                             uint4* st0, uint2* st1, uint32_t* ctl, uint32_t grid, hipStream_t s);
hipError_t launch_naive_mk(const MediumParams& m, const LaunchParams& L, hipStream_t s);
// naiveMK with the reference's compaction count (CVR_OPT_MK_COMPACTION 1):
// d_init over the tile's pixels, then one d_extend launch per bounce; `st`
// holds 3 float4 per pixel, `live` one flag, `ctl` the bounce's survivors.
struct MkCtl {
  uint32_t count;   // live paths after the bounce
  uint32_t max_id;  // highest live pixel id (the one end - begin - 1 drops)
};
hipError_t launch_mk_init(const MediumParams& m, const LaunchParams& L, uint32_t iteration, float4* st,
                          uint32_t* live, hipStream_t s);
hipError_t launch_mk_extend(const MediumParams& m, const LaunchParams& L, uint32_t iteration, uint32_t depth,
                            float4* st, uint32_t* live, MkCtl* ctl, hipStream_t s);
hipError_t launch_image_to_host(const float* src, float* dst, size_t n, float scale, hipStream_t s);
hipError_t launch_blocks_to_host(const float* src, float* dst, uint32_t w, uint32_t h, uint32_t rank, uint32_t world,
                                 float scale, hipStream_t s);
hipError_t launch_build_bounds(const float* density, uint32_t rx, uint32_t ry, uint32_t rz, uint32_t bshift,
                               float max_density, uint8_t* bounds, hipStream_t s, uint32_t format = 0);
// Sparse medium: cell-leaf pool (`coords`: 3 u32 leaf coordinates per slot,
// slot 0 the zero leaf) and brick words (`cell_slot`: per leaf, its slot or 0).
// `m` carries the leaf table/pools and the brick geometry (bshift <= 3).
hipError_t launch_build_sparse(const MediumParams& m, const uint32_t* coords, size_t n_cell_leaves,
                               const uint32_t* cell_slot, uint32_t bnz, float max_density, int unbounded,
                               float4* cells, uint32_t* sbounds, hipStream_t s);
hipError_t launch_build_cells(const float* density, uint32_t rx, uint32_t ry, uint32_t rz, float4* cells,
                              hipStream_t s, uint32_t format = 0);
// The half storage format (MediumParams::format 1; `format` above: `density` holds halves and
// the cells are written as 8 halves): n fp32 values -> n binary16, round to nearest even.
hipError_t launch_to_half(const float* src, void* dst, size_t n, hipStream_t s);
// The launch geometry of the medium build: every cap and run length the build launches and their
// kernels use, named once, so that cvr_debug_build_geometry (cvr.h) reports what runs.  Each
// kernel below a cap loops over its grid; the tests size their media from these to make it loop.
// (k_gradient's task cap and z run are the walk's: kWalkTaskCap, kWalkZ of cvr_gradient.h.)
constexpr uint32_t kScanGridCap = 2048;    // scan_grid: the value scans and k_classified, 8 workgroups per CU
constexpr uint32_t kStreamGridCap = 8192;  // stream_grid: k_fill_albedo, k_cell_leaf_flags, k_gather_leaves
constexpr uint32_t kScanSteps = 8, kScanTile = 256 * kScanSteps;  // flags per workgroup of the flag scan
constexpr uint32_t kScanSumsChunk = 1024;  // tile sums k_scan_sums takes per trip (its workgroup's size)
constexpr uint32_t kLeafRunLeaves = 32, kLeafRunVoxels = 8 * kLeafRunLeaves;  // x run of one k_leaf_flags task
constexpr uint32_t kLeafFlagsGridCap = 1u << 20;
constexpr uint32_t kToHalfGridCap = 8192;
constexpr uint32_t kBuildCellsGrid = 4096, kBuildBoundsGrid = 1024;  // fixed grids, each work-item looping
constexpr uint32_t kBuildSparseCellsGrid = 8192, kBuildSparseBoundsGrid = 4096;
// Media built from device memory (cvr_set_medium_device; cvr_medium_build.hip).  Every array below
// is device memory; the launches are asynchronous on s and none waits on another workgroup.
// What the value scans find, in device memory; the host sets ovf_* to ~0 and the rest to 0 first.
struct VoxelSource;  // below: the caller's arrays, or a scalar field and a transfer table
constexpr uint32_t kKeptSlots = 32;  // words a clipped build's kept-voxel count is spread over (MedScan::kept)
constexpr uint32_t kLabelSlots = 8;  // copies of a labelled build's 256 label counters, by the workgroup's index
struct MedScan {
  unsigned long long ovf_density;  // smallest index whose finite value rounds to +-inf in binary16 (format 1)
  unsigned long long ovf_albedo;   // the same over the albedo's r, g, b (index 4 voxel + channel)
  uint32_t max_bits;               // bits of max(0, every non-NaN density)
  uint32_t albedo_flags;           // bit 0: an rgb (format 1: rounded to half) differs from voxel 0's;
                                   // bit 1: a voxel's 16 bytes differ from voxel 0's
  uint32_t total[2];               // totals of the two flag scans (launch_flag_scan)
  // a clipped build: the voxels its clip keeps, added by the store or leaf-flag pass, a
  // workgroup's count to slot blockIdx.x % kKeptSlots; the host adds the slots
  unsigned long long kept[kKeptSlots];
};
hipError_t launch_scan_density(const float* density, size_t n, uint32_t format, MedScan* out, hipStream_t s);
hipError_t launch_scan_albedo(const float* albedo, size_t n, uint32_t format, MedScan* out, hipStream_t s);
// n albedo voxels of the context's grid (float4, format 1: 4 halves) set to `value`
hipError_t launch_fill_albedo(void* albedo, size_t n, uint32_t format, const float value[4], hipStream_t s);
// The leaf rule of cvr.h: flags[leaf] = the leaf exists (albedo null: by density alone); ln = ceil(res / 8).
// A classified source is launched with_albedo and also finds, of the classified values, what the
// two scans above find (scan; format as theirs); the arrays' source ignores both.
hipError_t launch_leaf_flags(const VoxelSource& src, bool with_albedo, const uint32_t res[3], const uint32_t ln[3],
                             uint32_t* flags, uint32_t format, MedScan* scan, hipStream_t s);
// flags[leaf] = the leaf or one of its 7 forward neighbours is in `table`
hipError_t launch_cell_leaf_flags(const uint32_t* table, const uint32_t ln[3], uint32_t* flags, hipStream_t s);
// Exclusive scan of n 0/1 flags, first two launches: sums (flag_scan_tiles(n) words) receives the
// number of set flags before each tile, *total their number.  The scatters below finish it.
size_t flag_scan_tiles(size_t n);
hipError_t launch_flag_scan(const uint32_t* flags, size_t n, uint32_t* sums, uint32_t* total, hipStream_t s);
// table[leaf] = slot or CVR_NO_LEAF, slots in leaf order; slot_leaf[slot] = leaf (*total words)
hipError_t launch_scatter_leaves(const uint32_t* flags, size_t n, const uint32_t* sums, uint32_t* table,
                                 uint32_t* slot_leaf, hipStream_t s);
// launch_build_sparse's cell_slot and coords (3 (*total + 1) words, slot 0 the zero leaf), and the
// empty-region mask's bits (emask: kEmaskWords zeroed words or null; super-bricks of 2^(3 + k_shift) cells)
hipError_t launch_scatter_cell_leaves(const uint32_t* flags, size_t n, const uint32_t* sums, const uint32_t ln[3],
                                      uint32_t* cell_slot, uint32_t* coords, uint32_t* emask, uint32_t k_shift,
                                      uint32_t shy, uint32_t shz, hipStream_t s);
// The stored leaves' pools from the grid (with_albedo false: no albedo), out-of-grid voxels (0, bg), format 1
// converted to binary16.  check non-null: nothing is stored; check->ovf_* receive the smallest pool
// index that overflows binary16.
hipError_t launch_gather_leaves(const VoxelSource& src, bool with_albedo, const uint32_t res[3], const uint32_t ln[3],
                                const uint32_t* slot_leaf, size_t n_leaves, const float bg[4], uint32_t format,
                                void* leaf_density, void* leaf_albedo, MedScan* check, hipStream_t s);
// Transfer functions (cvr_set_medium_scalar, cvr_classify_host).  The per-voxel classification
// cvr.h states: the one definition, compiled for the host and for the build kernels.  fp32 only,
// every operation in the written order (-ffp-contract=off, correctly rounded /), so both sides
// return the same bits.  table: n entries (r, g, b, density).  Returns (r, g, b, density): the
// voxel's albedo is (r, g, b, 1).
struct TransferParams {
  uint32_t n, flags;  // cvr_transfer_desc's: flags bit 0 CVR_TF_CEIL, bit 1 CVR_TF_DENSITY_U
  float lo, hi;
};
__host__ __device__ inline float4 transfer_classify(float s, const float4* table, const TransferParams& p) {
  const float u = unit_clamp(s, p.lo, p.hi);
  const float x = u * (float)(p.n - 1u);
  float4 e;
  if (p.flags & 1u) {
    const uint32_t c = (uint32_t)__builtin_ceilf(x), i = c < p.n - 1u ? c : p.n - 1u;
    e = table[i];
  } else {
    const uint32_t c = (uint32_t)__builtin_floorf(x), i = c < p.n - 2u ? c : p.n - 2u;
    const float f = x - (float)i;
    const float4 a = table[i], b = table[i + 1u];
    e.x = a.x + f * (b.x - a.x);
    e.y = a.y + f * (b.y - a.y);
    e.z = a.z + f * (b.z - a.z);
    e.w = a.w + f * (b.w - a.w);
  }
  if (p.flags & 2u) e.w = u;
  return e;
}
// The labelled classification (cvr.h: CVR_HAS_LABELS): the statement above on row `label` of a
// table of m rows of p.n entries, row 0 for a label the table has no row for.
__host__ __device__ inline float4 label_classify(float s, uint32_t label, const float4* table, uint32_t m,
                                                 const TransferParams& p) {
  const uint32_t j = label < m ? label : 0u;
  return transfer_classify(s, table + (size_t)j * p.n, p);
}
// One scalar voxel as the float the classification starts from (exact for the integer types)
__host__ __device__ inline float scalar_voxel(const void* scalar, uint32_t type, size_t i) {
  switch (type) {
    case 1: return (float)static_cast<const uint8_t*>(scalar)[i];
    case 2: return (float)static_cast<const uint16_t*>(scalar)[i];
    case 3: return (float)static_cast<const int16_t*>(scalar)[i];
    default: return static_cast<const float*>(scalar)[i];
  }
}
// Field statistics and value-gradient histograms (cvr_field_stats, cvr_field_histogram and their
// *_host statements; cvr_field.hip).  The coordinates are the classification's u and v, bit for
// bit (unit_clamp, cvr_gradient.h), and a bin is the nearest table node: the one definition for
// the host and the kernels, on the same terms as transfer_classify.
struct FieldBins {
  uint32_t n, m;  // value bins, gradient bins (m == 1: no gradient axis)
  float lo, hi, glo, ghi;
};
// The bin of coordinate c (0..1) on an axis of k nodes: the nearest node, ties upward, with no
// rounded c * (k - 1) + 0.5: f = x - (float)i0 is exact.
__host__ __device__ inline uint32_t field_bin(float c, uint32_t k) {
  const float x = c * (float)(k - 1u);
  const uint32_t fl = (uint32_t)__builtin_floorf(x), i0 = fl < k - 1u ? fl : k - 1u;
  const float f = x - (float)i0;
  const uint32_t b = i0 + (f >= 0.5f ? 1u : 0u);
  return b < k - 1u ? b : k - 1u;
}
// A float's bits as an integer that orders as the values do, -0 below +0 (NaNs lie outside
// [key(-inf), key(+inf)]), and back
__host__ __device__ inline uint32_t field_key(uint32_t bits) {
  return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__host__ __device__ inline uint32_t field_unkey(uint32_t key) {
  return key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu);
}
constexpr uint32_t kFieldKeyPosInf = 0xFF800000u, kFieldKeyNegInf = 0x007FFFFFu;  // field_key of +inf, -inf
// The launch geometry of the field kernels, named once (cvr_debug_field_geometry reports them)
constexpr uint32_t kFieldGrid1D = 2048;      // the 1-D histogram's grid cap (workgroups of 256)
constexpr uint32_t kFieldLdsBins = 16384;    // bins a workgroup-private LDS histogram holds (64 KB)
constexpr uint32_t kFieldMaxBins = 65536;    // the largest n * m
// The field as the kernels take it: res and the spacing's reciprocals
struct FieldSrc {
  const void* scalar = nullptr;
  uint32_t scalar_type = 0;
  uint32_t res[3] = {0u, 0u, 0u};
  GradientAxes axes;
};
// What the statistics pass finds, in device memory; the host sets kmin = kFieldKeyPosInf,
// kmax = kFieldKeyNegInf and the rest to 0 first.
struct FieldScan {
  uint32_t kmin, kmax;   // field_key of the smallest and the largest non-NaN value
  uint32_t gmax_bits;    // bits of the largest non-NaN gradient magnitude (>= +0: they order as the values)
  uint32_t pad;
  unsigned long long nan_values, nan_gradients;
};
// Asynchronous on s; none waits on another workgroup.  The histogram launch clears and then
// fills all n * m words of d_counts; m == 1 reads neither glo, ghi nor h1, h2.
hipError_t launch_field_stats(const FieldSrc& f, FieldScan* d_out, hipStream_t s);
hipError_t launch_field_histogram(const FieldSrc& f, const FieldBins& b, uint32_t* d_counts, hipStream_t s);
// Where the build stages take a voxel's values from: the caller's two arrays (scalar null;
// albedo null: none), or a scalar field of type scalar_type (cvr.h: CVR_SCALAR_*) classified
// through a table in device memory: the 1-D one by the value (tf), or, with `gradient`, the 2-D
// one by the value and the gradient magnitude (gtf; res is the field's, the stencil needs it), or,
// with `labels`, a table of label_rows rows of tf.n entries, the row chosen by the voxel's label
// byte (cvr.h: CVR_HAS_LABELS).
struct VoxelSource {
  const float* density = nullptr;
  const float* albedo = nullptr;
  const void* scalar = nullptr;
  uint32_t scalar_type = 0;
  const float4* table = nullptr;
  TransferParams tf{};
  bool gradient = false;
  uint32_t res[3] = {0u, 0u, 0u};
  GradientParams gtf{};
  // A labelled source: one label byte per voxel (device memory, any alignment), the table's rows,
  // and kLabelSlots x 256 zeroed words of device memory that the dense store pass or the leaf-flag
  // pass adds the kept voxels' label bytes to (label_counts[slot * 256 + byte]; the host adds the slots)
  const uint8_t* labels = nullptr;
  uint32_t label_rows = 0;
  uint32_t* label_counts = nullptr;
  // The clip region the build honours (cvr_clip.h; host memory, hi clamped to the grid), or null.
  // With one, every launch below that takes the source runs its clipped instance: a voxel the
  // region does not keep is (0, the unclipped voxel 0's albedo) and is not read.
  const ClipRegion* clip = nullptr;
  float clip_a0[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // with it: the unclipped source's albedo of voxel 0
};
// The arrays' source, dense, with a clip: one pass in the place of launch_scan_density and
// launch_scan_albedo (albedo null: the densities alone), of the clipped values, and one in the
// place of the copy or launch_to_half, which stores every voxel (albedo null: the density grid
// alone) and adds the kept voxels to scan->kept.  res is the grid's.
hipError_t launch_scan_clipped(const VoxelSource& src, const uint32_t res[3], uint32_t format, MedScan* out,
                               hipStream_t s);
hipError_t launch_store_clipped(const VoxelSource& src, const uint32_t res[3], uint32_t format, void* density,
                                void* albedo, MedScan* scan, hipStream_t s);
// Classified source, dense: one pass over the scalar field that finds what launch_scan_density and
// launch_scan_albedo find together, and one that stores every voxel's density and albedo
// (format 1: binary16) into the context's grids.  n = the voxels; a gradient source is walked by
// its res, z-planes marching through registers, with the same two results.
// With a clip (src.clip, src.res the grid's) the store adds the kept voxels to scan->kept.
hipError_t launch_scan_classified(const VoxelSource& src, size_t n, uint32_t format, MedScan* out, hipStream_t s);
hipError_t launch_store_classified(const VoxelSource& src, size_t n, uint32_t format, void* density, void* albedo,
                                   MedScan* scan, hipStream_t s);
// cvr_debug_fastdiv (tests): q[i] = fastdiv(u[i], f) on the device, u and q device arrays.
hipError_t launch_debug_fastdiv(FastDiv f, const uint32_t* u, uint32_t* q, size_t n, hipStream_t s);
hipError_t launch_tile_to_image(const float4* tile, uint32_t tw, uint32_t th, float4* image, uint32_t iw,
                                uint32_t ox, uint32_t oy, float scale, hipStream_t s);
// Adaptive sampling (cvr_adaptive_*).  The error metric of one pixel from its sums (cvr.h,
// cvr_block_error): the one definition, compiled for the host and for k_block_error.
//   m_c = S1_c / N, v_c = max(0, S2_c / N - m_c^2) / (N - 1),
//   e = sqrt(v_r + v_g + v_b) / (m_r + m_g + m_b + floor), all in fp64
// A NaN or infinite sum gives +inf (such a pixel never converges), a zero denominator 0.
__host__ __device__ inline double pixel_error(const float s1[3], const float s2[3], uint32_t n_samples, float floor) {
  const double N = (double)n_samples;
  double v = 0.0, m = (double)floor;
  for (int c = 0; c < 3; ++c) {
    const double a = (double)s1[c], b = (double)s2[c];
    if (!(a - a == 0.0) || !(b - b == 0.0)) return __builtin_huge_val();
    const double mc = a / N;
    const double d = b / N - mc * mc;
    v += (d > 0.0 ? d : 0.0) / (N - 1.0);
    m += mc;
  }
  if (m == 0.0) return 0.0;
  const double e = __builtin_sqrt(v) / m;
  return e == e ? e : __builtin_huge_val();
}
// errors[i] = the mean pixel_error over the 64 pixels of tile block blocks[i] (8x8 pixels,
// row-major block ids), each with n_samples samples; `moments` = tile + tile_px.
hipError_t launch_block_error(const float4* tile, uint32_t tile_px, uint32_t tile_w, const uint32_t* blocks,
                              uint32_t n, uint32_t n_samples, float floor, double* errors, hipStream_t s);
// k_tile_to_image with every pixel divided by its own 8x8 block's sample count (0: the pixel is 0);
// `image` is tile-sized device memory or the device address of a pinned host image.
hipError_t launch_tile_to_image_counts(const float4* tile, uint32_t tw, uint32_t th, const uint32_t* counts,
                                       float4* image, hipStream_t s);

// Denoiser (cvr_denoise*).  The per-pixel bodies of the filter cvr.h states: the one definition,
// compiled for the host (cvr_denoise_host) and for k_denoise_prepare / k_denoise_pass.  fp32
// only, every operation in the written order (-ffp-contract=off, correctly rounded / and sqrt),
// so both sides return the same bits.  An image pixel is (m_r, m_g, m_b, v); v < 0: invalid.
__host__ __device__ inline bool denoise_finite3(const float4 s) {
  return s.x - s.x == 0.0f && s.y - s.y == 0.0f && s.z - s.z == 0.0f;
}
__host__ __device__ inline float denoise_luma(float r, float g, float b) {
  return (0.2126f * r + 0.7152f * g) + 0.0722f * b;
}
// One pixel's samples: n_samples, or the count of its 8x8 block (counts: w / 8 entries per row).
__host__ __device__ inline uint32_t denoise_count(const uint32_t* counts, uint32_t n_samples, uint32_t w, uint32_t x,
                                                  uint32_t y) {
  return counts ? counts[(y >> 3) * (w >> 3) + (x >> 3)] : n_samples;
}
// Prepare: the sums s1, s2 of one pixel with n samples -> (mean rgb, variance of the mean's luminance).
__host__ __device__ inline float4 denoise_prepare(const float4 s1, const float4 s2, uint32_t n) {
  if (n < 2u || !denoise_finite3(s1) || !denoise_finite3(s2)) return make_float4(0.0f, 0.0f, 0.0f, -1.0f);
  const float N = (float)n, N1 = N - 1.0f;
  const float mr = s1.x / N, mg = s1.y / N, mb = s1.z / N;
  const float dr = s2.x / N - mr * mr, dg = s2.y / N - mg * mg, db = s2.z / N - mb * mb;
  const float vr = (dr > 0.0f ? dr : 0.0f) / N1, vg = (dg > 0.0f ? dg : 0.0f) / N1, vb = (db > 0.0f ? db : 0.0f) / N1;
  const float v = ((0.2126f * 0.2126f) * vr + (0.7152f * 0.7152f) * vg) + (0.0722f * 0.0722f) * vb;
  return make_float4(mr, mg, mb, v);
}
// One a-trous pass at pixel (x, y) of a w x h image, step `step`: the filtered pixel.  tap(qx, qy)
// returns the image's pixel at a coordinate inside the image (it is asked for no other), from
// wherever the caller keeps it: the order of the arithmetic does not depend on that.
// The guided filter (cvr_denoise_guided*): a valid centre's tap weight is divided once more, by g g
// with g = 1 + ((f_a f_a + f_z f_z) + f_o f_o) from the noise-free feature planes read at p and q
// (cvr.h); a sigma <= 0 leaves its term 0, and all three off give g = 1: the unguided bits.
struct DenoiseNoGuide {
  static constexpr bool on = false;
  __host__ __device__ float weight(float wt, size_t, size_t) const { return wt; }
};
struct DenoiseGuide {
  static constexpr bool on = true;
  const float* rgba;   // feat_rgba, 4 floats per pixel (device side: 16-byte aligned)
  const float* depth;  // feat_depth
  float sigma_albedo, sigma_depth, sigma_alpha;
  __host__ __device__ float4 feat(size_t i) const {
#ifdef __HIP_DEVICE_COMPILE__
    return reinterpret_cast<const float4*>(rgba)[i];
#else
    return make_float4(rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2], rgba[4 * i + 3]);
#endif
  }
  // the weight wt of tap q (pixel index iq) for centre p (pixel index ip)
  __host__ __device__ float weight(float wt, size_t ip, size_t iq) const {
    const float4 a = feat(ip), b = feat(iq);
    float fa = 0.0f, fz = 0.0f, fo = 0.0f;
    if (sigma_albedo > 0.0f) fa = ((fabsf(b.x - a.x) + fabsf(b.y - a.y)) + fabsf(b.z - a.z)) / sigma_albedo;
    if (sigma_depth > 0.0f) fz = fabsf(depth[iq] - depth[ip]) / sigma_depth;
    if (sigma_alpha > 0.0f) fo = fabsf(b.w - a.w) / sigma_alpha;
    const float g = 1.0f + ((fa * fa + fz * fz) + fo * fo);
    return wt / (g * g);
  }
};
template <class Tap, class Guide = DenoiseNoGuide>
__host__ __device__ __forceinline__ float4 denoise_pass_at(const Tap& tap, uint32_t w, uint32_t h, uint32_t x,
                                                           uint32_t y, uint32_t step, float sigma, float floor,
                                                           const Guide& guide = Guide{}) {
  const float G[3] = {0.25f, 0.5f, 0.25f};
  const float K[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
  const int iw = (int)w, ih = (int)h, px = (int)x, py = (int)y, s = (int)step;
  const float4 p = tap(px, py);
  const bool valid = !(p.w < 0.0f);
  float den = 1.0f, lp = 0.0f;
  if (valid) {
    float gs = 0.0f, gw = 0.0f;
    for (int j = -1; j <= 1; ++j)
      for (int i = -1; i <= 1; ++i) {
        const int qx = px + i, qy = py + j;
        if (qx < 0 || qx >= iw || qy < 0 || qy >= ih) continue;
        const float vq = tap(qx, qy).w;
        if (vq < 0.0f) continue;
        const float wt = G[j + 1] * G[i + 1];
        gs += wt * vq;
        gw += wt;
      }
    den = sigma * sqrtf(gs / gw) + floor;
    lp = denoise_luma(p.x, p.y, p.z);
  }
  float cr = 0.0f, cg = 0.0f, cb = 0.0f, vs = 0.0f, ws = 0.0f;
  for (int j = -2; j <= 2; ++j)
    for (int i = -2; i <= 2; ++i) {
      const int qx = px + s * i, qy = py + s * j;
      if (qx < 0 || qx >= iw || qy < 0 || qy >= ih) continue;
      const float4 q = tap(qx, qy);
      if (q.w < 0.0f) continue;
      float wt = K[j + 2] * K[i + 2];
      if (valid) {
        const float a = fabsf(denoise_luma(q.x, q.y, q.z) - lp) / den;
        const float u = 1.0f + a * a;
        wt = wt / (u * u);
        if (Guide::on) wt = guide.weight(wt, (size_t)py * w + (size_t)px, (size_t)qy * w + (size_t)qx);
      }
      cr += wt * q.x;
      cg += wt * q.y;
      cb += wt * q.z;
      vs += (wt * wt) * q.w;
      ws += wt;
    }
  if (ws == 0.0f) return make_float4(0.0f, 0.0f, 0.0f, -1.0f);
  return make_float4(cr / ws, cg / ws, cb / ws, vs / (ws * ws));
}
// The image in plain memory, row-major: the host statement and the kernels' global loads.
struct DenoiseImage {
  const float4* src;
  uint32_t w;
  __host__ __device__ float4 operator()(int qx, int qy) const { return src[(size_t)qy * w + (size_t)qx]; }
};
template <class Guide = DenoiseNoGuide>
__host__ __device__ __forceinline__ float4 denoise_pass(const float4* src, uint32_t w, uint32_t h, uint32_t x,
                                                        uint32_t y, uint32_t step, float sigma, float floor,
                                                        const Guide& guide = Guide{}) {
  return denoise_pass_at(DenoiseImage{src, w}, w, h, x, y, step, sigma, floor, guide);
}
// The output pixel from the last pass's result f, the pixel's sum s1 and its n samples.
__host__ __device__ inline float4 denoise_final(const float4 f, const float4 s1, uint32_t n) {
  const float a = n >= 2u ? s1.w / (float)n : 0.0f;
  return f.w < 0.0f ? make_float4(0.0f, 0.0f, 0.0f, a) : make_float4(f.x, f.y, f.z, a);
}
// Device side (cvr_denoise.hip): prepare into `img`, or one pass src -> dst; the last pass (sum
// non-null) stores denoise_final into out_rgba (device memory or the device address of pinned
// host memory) and the filtered v, -1 for an invalid pixel, into out_var (may be null).
hipError_t launch_denoise_prepare(const float4* sum, const float4* m2, uint32_t w, uint32_t h, uint32_t n_samples,
                                  const uint32_t* counts, float4* img, hipStream_t s);
// guide non-null: the guided instances of the same kernels.
hipError_t launch_denoise_pass(const float4* src, float4* dst, uint32_t w, uint32_t h, uint32_t step, float sigma,
                               float floor, hipStream_t s, const DenoiseGuide* guide = nullptr);
hipError_t launch_denoise_last(const float4* src, uint32_t w, uint32_t h, uint32_t step, float sigma, float floor,
                               const float4* sum, uint32_t n_samples, const uint32_t* counts, float4* out_rgba,
                               float* out_var, hipStream_t s, const DenoiseGuide* guide = nullptr);

}  // namespace cvr
