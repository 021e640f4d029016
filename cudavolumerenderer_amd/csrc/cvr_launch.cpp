// cvr_launch.cpp - the render launch behind the C ABI: which scheduler runs a kernel id and at what
// grid, the work orders, the plan of a launch (plan_launch) and the launch itself, with the host
// loops of the schedulers that need one (the kernels: cvr_wpool.hip, cvr_persistent.hip,
// cvr_pool.hip, cvr_wavefront.hip, cvr_kernels.hip).
//
// Reference map:
//   RenderKernelLauncher / VolPTKernelLauncher  RenderKernelLauncher.h:20-174,
//                                                RenderKernelLauncher.cu:86-361
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "cvr_host.h"

namespace cvr {
// d_work layout: cvr_kernels.h (stats, debug counters, queue heads)
constexpr size_t kWorkBytes = kWorkBytesBase;

// Scheduler that implements each persistent kernel id (results
// depend only on the kernel id's scatter offset and per-tile seed, quirks
// Q2/Q6, so every id may run on any scheduler).  Round 5: every persistent id
// runs the wave-private LDS pool by default, its ballot/prefix compaction of
// finished segments being the streaming kernels' compaction
// (StreamingVolPTsk_kernel.cuh:176-216, StreamingVolPTmk_kernel.cuh:218-252)
// at wave granularity; sortingSK's event batches run sorted by kind; naiveSK
// (one thread per path in the reference, NaiveVolPTsk_kernel.cuh:17-87) runs
// there too: its image is fixed by its Rng(path_id) streams, scatter -eps and
// per-tile seeds, not by the thread mapping (C2: 4.5 vs 26.8 ms as one path
// per work-item).  The structural restatements stay behind CVR_OPT_SCHEDULER:
// 4 one path per work-item (k_naive, naiveSK's own mapping), 2 the workgroup
// pool with bulk compaction phases (StreamingVolPTsk's block streaming, 3-4x
// slower on C2), 1 the multi-kernel wavefront pair (StreamingVolPTmk's
// device-wide compaction), 0 one path per lane of a persistent wave.  naiveMK
// always runs its own kernels (k_naive_mk: per-bounce reseeding, Q12).
int scheduler_for(const cvr_ctx* c) {
  if (c->scheduler >= 0) return c->scheduler;
  return 3;
}

// Scatter origin offset per scheduler: every kernel subtracts
// d*eps at a real collision except single-thread regeneration
// (RegenerationVolPTsk_kernel.cuh:212).
bool scatter_eps_for(const cvr_ctx* c) {
  if (c->scatter_eps >= 0) return c->scatter_eps != 0;
  return c->kernel != CVR_KERNEL_REGENERATION_SK;
}

// streamingSK's default variant sorts its rays by Morton code (Q14,
// StreamingVolPTsk_kernel.cuh:188-216); here the pool scheduler's track order
// does so when CVR_OPT_MORTON is 1.  Off by default: the sort makes the pool
// kernel 8% slower on C2 and 7% on C3.
static bool morton_for(const cvr_ctx* c) { return c->morton > 0; }

// dense and sparse at the default (split slots: DESIGN.md §6)
static int wpool_waves_for(const cvr_ctx* c) { return c->wpool_waves ? c->wpool_waves : cvr::kWpoolWaves; }
// What the context's wave-pool launch asks of k_wpool; cvr::wpool_select says which instance runs it, if any.
static cvr::WpoolRequest wpool_request(const cvr_ctx* c, bool record, bool flush) {
  const bool sparse = c->m.leaves != nullptr;
  return {scatter_eps_for(c), wpool_waves_for(c), sparse, !sparse && c->m.cells && c->m.bounds,
          c->m.albedo_uniform != 0u, c->m.format != 0u, c->kernel == CVR_KERNEL_NAIVE_MK, c->count_words != 0,
          c->moments != 0, record, flush, c->have_env};
}
// The generic instance of a layout at the context's budget (never refused): do_init's grids, every such instance's wpg.
static cvr::WpoolInstance wpool_generic(const cvr_ctx* c, bool sparse) {
  cvr::WpoolInstance k{};
  (void)cvr::wpool_select({scatter_eps_for(c), wpool_waves_for(c), sparse}, &k);
  return k;
}

// naiveMK runs the wave pool (k_wpool's kMedMK instances: d_init + d_extend per path, RNG re-seeded per bounce;
// C2 27.5 -> ~4.5 ms) unless another scheduler, a budget without such an instance or the reference's per-bounce
// compaction is asked for.  The request is the walk alone: launch refuses what else no instance runs.
static bool mk_on_wpool(const cvr_ctx* c) {
  cvr::WpoolInstance k;
  return c->kernel == CVR_KERNEL_NAIVE_MK && scheduler_for(c) == 3 && !c->mk_compaction &&
         cvr::wpool_select({true, wpool_waves_for(c), false, false, false, false, /*naive_mk*/ true}, &k);
}

// What the context has that the half-format (kForHalf), the moments instances (kForMoments: generic dense / fp32
// sparse layout) or the environment instances (kForEnv) do not run with: the first entry of the feature's that
// holds, or null.
const char* wpool_refusal(const cvr_ctx* c, unsigned feature) {
  const struct { unsigned features; bool holds; const char* text; } list[] = {
      {kForMoments, c->external_out, "a caller's output buffer (cvr_set_output)"},
      {kForMoments | kForEnv, c->kernel == CVR_KERNEL_NAIVE_MK, "kernel id naiveMK"},
      {kForAll, c->rng_binding != 0, "CVR_OPT_RNG_BINDING 1"},
      {kForAll, scheduler_for(c) != 3, "a scheduler other than the wave pool (CVR_OPT_SCHEDULER 3)"},
      {kForAll, wpool_waves_for(c) != cvr::kWpoolWaves, "CVR_OPT_WAVES other than 5"},
      {kForAll, c->mk_compaction != 0, "CVR_OPT_MK_COMPACTION 1"},
      {kForAll, c->count_words != 0, "CVR_OPT_COUNT_WORDS 1"},
      {kForMoments, c->m.leaves && c->m.format != 0u, "a sparse half medium"},
  };
  for (const auto& e : list)
    if ((e.features & feature) && e.holds) return e.text;
  return nullptr;
}

// Wave-pool grid of a launch of n_paths (one wave per workgroup): CVR_OPT_GRID,
// else the occupancy grid, of which a small launch takes a part.  A launch of
// fewer than 64 paths per wave (C1: 262 K paths) ends mostly in ramp-up and
// ramp-down at the full grid: half the grid alone, a quarter with renders in
// flight (the other renders fill the rest; profiles/round2/overlap_c1.log:
// 0.228 vs 0.287 ms alone, 0.094 vs 0.149 ms per render with three in flight).
// With renders in flight (CVR_OPT_INFLIGHT > 1) a launch of fewer than 2048
// paths per wave at the full grid (the 8- and 4-GPU block shards of C2) takes
// half the grid, so each wave gets twice the paths (1/8 shard 0.700 vs 0.735
// ms per render, profiles/round2/overlap_small_shards.log; round 4, three in
// flight: 1/4 shard 1.282 vs 1.320 ms, 1/8 shard 0.724 vs 0.768 at 3/4 grid,
// profiles/round4/shard_grid.log); alone the full grid is faster.
// The grid counts waves, in whole workgroups of the instance (cvr::wpool_wpg).
static uint32_t wpool_launch_grid(const cvr_ctx* c, uint64_t n_paths) {
  const uint32_t wpg = cvr::wpool_wpg(wpool_generic(c, c->m.leaves != nullptr));
  auto whole = [wpg](uint32_t g) { return std::max(wpg, g / wpg * wpg); };
  if (c->grid_override) return whole(c->grid_override);
  const uint32_t full = (uint32_t)(c->m.leaves ? c->wpool_grid_sparse : c->wpool_grid);
  const uint32_t half = std::max(1u, full / 2), quarter = std::max(1u, full / 4);
  if (n_paths < 64ull * full) return whole(c->inflight > 1 ? quarter : half);
  if (c->inflight > 1 && n_paths < 2048ull * full) return whole(half);
  return whole(full);
}

// FastDiv constants for d >= 1 (cvr_walk.h fastdiv): l = ceil(log2 d),
// m = floor(2^32 (2^l - d) / d) + 1, s1 = min(l, 1), s2 = max(l - 1, 0) (sh = s1 | s2 << 8).
FastDiv make_fastdiv(uint32_t d) {
  if (d == 0) d = 1;
  uint32_t l = 0;
  while (l < 32 && (1ull << l) < d) ++l;
  cvr::FastDiv f;
  f.m = (uint32_t)((((1ull << l) - d) << 32) / d + 1);
  f.sh = (l < 1 ? l : 1) | ((l > 1 ? l - 1 : 0) << 8);
  return f;
}

// The plan of paths [first, first + count) of the tile (sharded: this context's shard of them), short of
// the wave pool's part (plan_launch).
static LaunchPlan fill_launch(const cvr_ctx* c, const LaunchArgs& a, uint64_t first, uint64_t count, bool sharded) {
  LaunchPlan plan;
  plan.first = first;
  plan.count = count;
  cvr::LaunchParams& L = plan.L;
  const uint32_t shard_world = sharded ? c->shard_world : 1u;
  const uint64_t P0 = (uint64_t)(uint32_t)((float)c->tile_w * (float)c->tile_h);
  // the persistent schedulers take work units through unit_to_path (pixel-block order); naiveSK/MK
  // and the wavefront pair map launch index -> path id directly
  const bool queued = (c->kernel != CVR_KERNEL_NAIVE_MK || mk_on_wpool(c)) && scheduler_for(c) != 1 &&
                      scheduler_for(c) != kSchedPerItem &&
                      c->rng_binding == 0;
  const bool block_order = queued && c->order && P0 && first % P0 == 0 && count % P0 == 0 && count > 0 &&
                           count / P0 <= (1ull << 20) && c->tile_w % 8 == 0 && c->tile_h % 8 == 0;
  if (shard_world > 1 && !block_order) {  // no block order: a contiguous share of the path ids
    const uint64_t base = count / c->shard_world, rem = count % c->shard_world;
    first += c->shard_rank * base + std::min<uint64_t>(c->shard_rank, rem);
    count = base + (c->shard_rank < rem ? 1 : 0);
  }
  memcpy(L.M, c->inv_view, sizeof(L.M));
  L.r2v[0] = c->r2v[0];
  L.r2v[1] = c->r2v[1];
  L.full_res[0] = c->full_res[0];
  L.full_res[1] = c->full_res[1];
  L.tile_res[0] = (float)c->tile_w;  // copyResolution(make_float2(res.x, res.y))
  L.tile_res[1] = (float)c->tile_h;
  L.off[0] = c->off[0];
  L.off[1] = c->off[1];
  L.tile_px = (uint32_t)(L.tile_res[0] * L.tile_res[1]);
  L.tile_w = (uint32_t)L.tile_res[0];
  L.path_first = (uint32_t)first;
  L.path_count = (uint32_t)count;
  L.seed_base = c->seed;
  L.max_segments = c->max_segments;
  L.out = a.out ? a.out : c->d_out;
  L.queue = reinterpret_cast<unsigned int*>(c->d_work + kWorkQueues);
  L.stats = reinterpret_cast<unsigned long long*>(c->d_work + kWorkStats);
  L.chunk = c->chunk ? c->chunk : 256;
  L.ev_thresh = c->ev_thresh ? c->ev_thresh : 1;
  L.tail = c->pool_tail;
  L.batch = c->swap_batch;
  L.naive_mk = (c->kernel == CVR_KERNEL_NAIVE_MK ? 1u : 0u) | (morton_for(c) ? 2u : 0u);
  // work order (see LaunchParams): pixel blocks with samples innermost, one
  // contiguous band of blocks per queue, when the launch covers whole samples
  const uint64_t P = L.tile_px;
  // (at most 2^20 samples: cvr_walk.h unit_to_path's pixel-of-unit division)
  const bool aligned = P && first % P == 0 && count % P == 0 && count > 0 && count / P <= (1ull << 20);
  L.blk_off = 0;
  L.blk_stride = 1;
  if (c->order && aligned && c->tile_w % 8 == 0 && c->tile_h % 8 == 0) {
    L.order = 1;
    L.samples = (uint32_t)(count / P);
    L.blocks_x = c->tile_w / 8;
    L.n_blocks = (uint32_t)(P / 64);
    if (c->active_on) {
      // the active block list: the launch's blocks are exactly the listed tile blocks, which reach
      // the kernel as block_perm (launch, ensure_active_order); blk_off 0, blk_stride 1
      L.n_blocks = (uint32_t)c->active.size();
      L.path_count = L.n_blocks * 64u * L.samples;
    } else if (shard_world > 1 && block_order) {  // blocks shard_rank, shard_rank + world, ...
      L.blk_off = c->shard_rank;
      L.blk_stride = c->shard_world;
      L.n_blocks = L.n_blocks > c->shard_rank ? (L.n_blocks - c->shard_rank + c->shard_world - 1) / c->shard_world : 0;
      L.path_count = L.n_blocks * 64u * L.samples;
    } else if (a.band.count && block_order && a.band.first < L.n_blocks) {  // cvr_render_frame's band
      L.blk_off = a.band.first;
      L.n_blocks = std::min(a.band.count, L.n_blocks - a.band.first);
      L.path_count = L.n_blocks * 64u * L.samples;
    }
    uint32_t bands = c->n_queues < L.n_blocks ? c->n_queues : L.n_blocks;
    if (bands == 0) bands = 1;
    // sub-queues per band: the wave pool only, each with at least one block
    // Sub-queues per band (8 by default: C2 5.03 vs 5.07 ms with one, manix 2048^2 28.9 vs
    // 29.2; C3 prefers one, 5.56 vs 5.60; profiles/round3/ab/sub3_*.log, c4sub.log)
    uint32_t sub = scheduler_for(c) == 3 ? c->subqueues : 1u;
    while (sub > 1 && bands * sub > L.n_blocks) --sub;
    L.sub = sub;
    L.n_queues = bands * sub;
  } else {
    L.order = 0;
    L.samples = 0;
    L.blocks_x = 0;
    L.n_blocks = 0;
    L.n_queues = 1;
    L.sub = 1;
  }
  L.div_queues = make_fastdiv(L.n_queues);
  // (a user table is ignored while a block list is active: the list itself travels as block_perm)
  L.block_perm = (L.order == 1 && !c->active_on && c->d_block_perm && c->block_perm_n == L.n_blocks) ? c->d_block_perm
                                                                                                       : nullptr;
  L.div_tile_px = make_fastdiv(L.tile_px);
  L.div_tile_w = make_fastdiv(L.tile_w);
  L.div_block = make_fastdiv(64u * L.samples);
  L.div_blocks_x = make_fastdiv(L.blocks_x);
  plan.block_order = block_order;
  return plan;
}

LaunchParams trace_params(const cvr_ctx* c, uint32_t first, uint32_t count) {
  return fill_launch(c, LaunchArgs{}, first, count, /*sharded=*/false).L;
}

// The medium as the kernels see it for this context's options: with the Q4
// fix (CVR_OPT_WORLD_TO_AABB 1) the Woodcock coordinate is (p - min) scaled by
// (res - 1)/extent instead of p - min/extent (cvr_walk.h MediumParams::gx).
cvr::MediumParams launch_medium(const cvr_ctx* c) {
  cvr::MediumParams m = c->m;
  if (!c->empty_mask) m.emask = nullptr;  // every super-brick loads its words
  if (c->world_to_aabb) {
    const float ex = m.bmax.x - m.bmin.x, ey = m.bmax.y - m.bmin.y, ez = m.bmax.z - m.bmin.z;
    m.shift = m.bmin;
    m.gx = m.agx / ex;
    m.gy = m.agy / ey;
    m.gz = m.agz / ez;
  }
  return m;
}

// First block of queue q of a launch (LaunchParams::n_queues; cvr_walk.h queue_blocks_begin).
static uint32_t queue_begin(const cvr::LaunchParams& L, uint32_t q) {
  return (uint32_t)((uint64_t)L.n_blocks * q / L.n_queues);
}
// First block of XCD band b (n_queues / sub bands of sub queues each).
static uint32_t band_begin(const cvr::LaunchParams& L, uint32_t b) { return queue_begin(L, b * L.sub); }

int do_init(cvr_ctx* c) {
  if (c->inited) return CVR_OK;
  int r = ensure_device(c);
  if (r) return r;
  hipDeviceProp_t prop;
  HIP_TRY(c, hipGetDeviceProperties(&prop, c->device));
  c->cu_count = prop.multiProcessorCount;
  int bpc = 0;
  HIP_TRY(c, cvr::persistent_occupancy(scatter_eps_for(c), c->waves, &bpc));
  if (bpc < 1) bpc = 1;
  c->persistent_grid = bpc * c->cu_count;
  int pbpc = 0;
  HIP_TRY(c, cvr::pool_occupancy(scatter_eps_for(c), &pbpc));
  if (pbpc < 1) pbpc = 1;
  c->pool_grid = pbpc * c->cu_count;
  int wbpc = 0;
  HIP_TRY(c, cvr::wpool_occupancy(wpool_generic(c, false), &wbpc));
  if (wbpc < 1) wbpc = 1;
  c->wpool_grid = wbpc * c->cu_count;
  HIP_TRY(c, cvr::wpool_occupancy(wpool_generic(c, true), &wbpc));
  if (wbpc < 1) wbpc = 1;
  c->wpool_grid_sparse = wbpc * c->cu_count;
  int tbpc = 0;
  HIP_TRY(c, cvr::wf_track_occupancy(&tbpc));
  if (tbpc < 1) tbpc = 1;
  c->track_grid = tbpc * c->cu_count;
  c->inited = true;
  return CVR_OK;
}

constexpr uint32_t kAliveRing = 8;

// Carve the SoA pool + per-wave cursors/stat rows out of one allocation.
static int ensure_pool(cvr_ctx* c, uint32_t n) {
  n = (n + 255u) & ~255u;
  const uint32_t ev_waves = n / 64u;
  const uint32_t tr_waves = (uint32_t)c->track_grid * 4u;
  const size_t slot_bytes = 19 * sizeof(uint32_t);  // 11 floats + 6 rng + img + meta
  const size_t need = (size_t)n * slot_bytes + (size_t)ev_waves * 8 + 256 + kAliveRing * 4 + 256 +
                      (size_t)(ev_waves + tr_waves) * 64 + 4096;
  if (need > c->pool_bytes) {
    if (c->d_pool) (void)hipFree(c->d_pool);
    c->d_pool = nullptr;
    c->pool_bytes = 0;
    HIP_TRY(c, hipMalloc(&c->d_pool, need));
    c->pool_bytes = need;
  }
  if (!c->h_alive) HIP_TRY(c, hipHostMalloc(&c->h_alive, kAliveRing * sizeof(unsigned int), hipHostMallocDefault));
  unsigned char* p = c->d_pool;
  auto take = [&](size_t bytes) {
    unsigned char* r = p;
    p += (bytes + 255) & ~(size_t)255;
    return r;
  };
  cvr::WfPool& P = c->pool;
  float** fl[] = {&P.ox, &P.oy, &P.oz, &P.dx, &P.dy, &P.dz, &P.tx, &P.ty, &P.tz, &P.dist, &P.t};
  for (float** f : fl) *f = reinterpret_cast<float*>(take((size_t)n * 4));
  uint32_t** ui[] = {&P.r0, &P.r1, &P.r2, &P.r3, &P.r4, &P.rd, &P.img, &P.meta};
  for (uint32_t** u : ui) *u = reinterpret_cast<uint32_t*>(take((size_t)n * 4));
  P.cursor = reinterpret_cast<uint32_t*>(take((size_t)ev_waves * 8));
  P.head = reinterpret_cast<unsigned int*>(take(256));
  P.alive = reinterpret_cast<unsigned int*>(take(kAliveRing * 4));
  P.stats_events = reinterpret_cast<unsigned long long*>(take((size_t)ev_waves * 64));
  P.stats_track = reinterpret_cast<unsigned long long*>(take((size_t)tr_waves * 64));
  P.n = n;
  c->pool_cap = n;
  return CVR_OK;
}

// The wavefront render of one launch: events / track alternate until no
// slot is alive.  The host polls the alive flags every few iterations.
static int wf_render(cvr_ctx* c, const cvr::LaunchParams& L, bool eps) {
  uint32_t n = L.path_count < c->pool_max ? L.path_count : c->pool_max;
  if (n < 256) n = 256;
  int r = ensure_pool(c, n);
  if (r) return r;
  cvr::WfPool P = c->pool;
  const uint32_t ev_waves = P.n / 64u;
  const uint32_t tr_waves = (uint32_t)c->track_grid * 4u;
  hipStream_t s = c->stream;
  HIP_TRY(c, hipMemsetAsync(P.meta, 0, (size_t)P.n * 4, s));  // WF_FREE
  HIP_TRY(c, hipMemsetAsync(P.cursor, 0, (size_t)ev_waves * 8, s));
  HIP_TRY(c, hipMemsetAsync(P.head, 0, 256, s));
  HIP_TRY(c, hipMemsetAsync(P.stats_events, 0, (size_t)ev_waves * 64, s));
  HIP_TRY(c, hipMemsetAsync(P.stats_track, 0, (size_t)tr_waves * 64, s));
  uint32_t it = 0;
  bool done = false;
  if (c->wf_timing && c->it_events.empty()) {
    c->it_events.resize(3 * 512);
    for (auto& e : c->it_events) HIP_TRY(c, hipEventCreate(&e));
  }
  double track_ms = 0, events_ms = 0;
  uint32_t timed_its = 0;
  while (!done) {
    cvr::WfPool Pi = P;
    Pi.alive = P.alive + (it % kAliveRing);
    HIP_TRY(c, hipMemsetAsync(Pi.alive, 0, 4, s));
    const bool tm = c->wf_timing && timed_its < 512;
    if (tm) HIP_TRY(c, hipEventRecord(c->it_events[3 * timed_its], s));
    HIP_TRY(c, cvr::wf_launch_events(launch_medium(c), L, Pi, eps, s));
    if (tm) HIP_TRY(c, hipEventRecord(c->it_events[3 * timed_its + 1], s));
    HIP_TRY(c, cvr::wf_launch_track(launch_medium(c), L, Pi, (uint32_t)c->track_grid, s));
    if (tm) {
      HIP_TRY(c, hipEventRecord(c->it_events[3 * timed_its + 2], s));
      ++timed_its;
    }
    HIP_TRY(c, hipMemcpyAsync(c->h_alive + (it % kAliveRing), Pi.alive, 4, hipMemcpyDeviceToHost, s));
    ++it;
    if (it % 4 == 0) {
      HIP_TRY(c, hipStreamSynchronize(s));
      for (uint32_t k = it - 4; k < it; ++k)
        if (c->h_alive[k % kAliveRing] == 0) done = true;
    }
    if (it > 100000) return set_err(&c->err, CVR_ERR_STATE, "wavefront render did not converge");
  }
  for (uint32_t k = 0; k < timed_its; ++k) {
    float a = 0, b = 0;
    HIP_TRY(c, hipEventElapsedTime(&a, c->it_events[3 * k], c->it_events[3 * k + 1]));
    HIP_TRY(c, hipEventElapsedTime(&b, c->it_events[3 * k + 1], c->it_events[3 * k + 2]));
    events_ms += a;
    track_ms += b;
  }
  // fold the per-wave counters into the context's 8 stats words
  unsigned long long* stats = reinterpret_cast<unsigned long long*>(c->d_work + kWorkStats);
  HIP_TRY(c, cvr::wf_launch_reduce(P.stats_events, ev_waves, stats, s));
  HIP_TRY(c, cvr::wf_launch_reduce(P.stats_track, tr_waves, stats + 8, s));
  c->last_iterations = it;
  c->last_track_ms = track_ms;
  c->last_events_ms = events_ms;
  return CVR_OK;
}

// naiveMK with the reference's compaction count (quirk Q11 reproduced,
// CVR_OPT_MK_COMPACTION 1): NaiveVolPTmk::launchRender / extend
// (RenderKernelLauncher.cu:183-272).  Per iteration: d_init over the tile,
// then bounces while the processed count is non-zero; after each bounce the
// count is (live paths) - 1 and the live path with the highest pixel id (last
// in the stable remove_if's output) is never extended again.  A bounce that
// leaves no live path makes the reference's uint count wrap to 2^32 - 1 (its
// next extend reads stale active-list entries, its remove_if runs off the
// array): reported as CVR_ERR_STATE.  One host sync per bounce, as the
// reference's thrust call.
static int mk_reference_render(cvr_ctx* c, const cvr::LaunchParams& L) {
  if (L.path_first != 0 || L.tile_px == 0 || L.path_count % L.tile_px != 0 || c->shard_world != 1)
    return set_err(&c->err, CVR_ERR_UNSUPPORTED,
                   "naiveMK with the reference compaction renders whole tiles only (no path range / shard)");
  const uint32_t iters = L.path_count / L.tile_px;
  const cvr::MediumParams m = launch_medium(c);
  float4* st = nullptr;
  uint32_t* live = nullptr;
  cvr::MkCtl* ctl = nullptr;
  HIP_TRY(c, hipMalloc(&st, (size_t)L.tile_px * 3 * sizeof(float4)));
  hipError_t e = hipMalloc(&live, (size_t)L.tile_px * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMalloc(&ctl, sizeof(cvr::MkCtl));
  int r = CVR_OK;
  for (uint32_t it = 0; it < iters && e == hipSuccess && r == CVR_OK; ++it) {
    e = cvr::launch_mk_init(m, L, it, st, live, c->stream);
    uint64_t n_processed = L.tile_px;
    for (uint32_t depth = 0; n_processed != 0 && e == hipSuccess; ++depth) {
      if (e == hipSuccess) e = hipMemsetAsync(ctl, 0, sizeof(cvr::MkCtl), c->stream);
      if (e == hipSuccess) e = cvr::launch_mk_extend(m, L, it, depth, st, live, ctl, c->stream);
      cvr::MkCtl h{};
      if (e == hipSuccess) e = hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, c->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
      if (e != hipSuccess) break;
      if (h.count == 0) {
        r = set_err(&c->err, CVR_ERR_STATE,
                    "naiveMK reference compaction (Q11): iteration %u bounce %u left no live path, so "
                    "end - begin - 1 underflows (RenderKernelLauncher.cu:271)",
                    it, depth);
        break;
      }
      n_processed = h.count - 1u;
      e = hipMemsetAsync(live + h.max_id, 0, sizeof(uint32_t), c->stream);  // dropped, never extended again
    }
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(st);
  if (live) (void)hipFree(live);
  if (ctl) (void)hipFree(ctl);
  if (r) return r;
  if (e != hipSuccess) return set_err(&c->err, CVR_ERR_HIP, "naiveMK reference compaction: %s", hipGetErrorString(e));
  return CVR_OK;
}

// streamingMK with the thread-bound RNG (CVR_OPT_RNG_BINDING 1):
// StreamingVolPTmk::launchRender (RenderKernelLauncher.cu:435-470).  Per
// iteration d_regenerate fills the slots from n_active on, n_active is reset,
// the slot buffers swap and d_extend runs one segment per active path (all of
// them once the head has passed the last path) and compacts the survivors;
// the host reads n_active and the head back, one sync per iteration as the
// reference.  The RNG states stay with the threads (cvr_kernels.hip
// k_smk_extend).  Buffers: 2 x 3 float4 + 2 flags per slot, 24 bytes of RNG
// state per thread and two counters, carved from one allocation that stays
// with the context (grown only when the grid grows).  Like the reference's
// host loop, a call blocks the host until the render has ended.
static int smk_thread_render(cvr_ctx* c, const cvr::LaunchParams& L, uint32_t grid) {
  if (L.path_count == 0) return CVR_OK;
  const size_t n = (size_t)grid * 256u;
  const cvr::MediumParams m = launch_medium(c);
  if (c->smk_n < n) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->d_smk) (void)hipFree(c->d_smk);
    c->d_smk = nullptr;
    c->smk_n = 0;
    // float4 slots | uint4 states | uint2 states | flags | counters (every part 16-byte aligned)
    const size_t bytes = 6 * n * sizeof(float4) + n * sizeof(uint4) + n * sizeof(uint2) + ((2 * n + 15) & ~(size_t)15) + 16;
    HIP_TRY(c, hipMalloc(&c->d_smk, bytes));
    c->smk_n = n;
  }
  unsigned char* p = c->d_smk;
  float4* slots = reinterpret_cast<float4*>(p);
  p += 6 * n * sizeof(float4);
  uint4* st0 = reinterpret_cast<uint4*>(p);
  p += n * sizeof(uint4);
  uint2* st1 = reinterpret_cast<uint2*>(p);
  p += n * sizeof(uint2);
  uint8_t* act = p;
  p += (2 * n + 15) & ~(size_t)15;
  uint32_t* ctl = reinterpret_cast<uint32_t*>(p);
  hipError_t e = hipMemsetAsync(ctl, 0, 2 * sizeof(uint32_t), c->stream);  // d_n_active = head = 0
  cvr::SmkSlots buf[2] = {{slots, slots + n, slots + 2 * n, act}, {slots + 3 * n, slots + 4 * n, slots + 5 * n, act + n}};
  int cur = 0;  // the buffer d_regenerate writes and the next d_extend reads
  uint32_t h[2] = {(uint32_t)n, 0u};
  uint64_t it = 0;
  int r = CVR_OK;
  while (e == hipSuccess && (h[0] > 0u || h[1] < L.path_count)) {
    if (++it > 100000000ull) {
      r = set_err(&c->err, CVR_ERR_STATE, "thread-bound streamingMK did not finish");
      break;
    }
    e = cvr::launch_smk_regen(L, buf[cur], st0, st1, ctl, grid, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(ctl, 0, sizeof(uint32_t), c->stream);  // d_n_active = 0
    if (e == hipSuccess) e = cvr::launch_smk_extend(m, L, buf[cur], buf[cur ^ 1], st0, st1, ctl, grid, c->stream);
    cur ^= 1;
    if (e == hipSuccess) e = hipMemcpyAsync(h, ctl, sizeof(h), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  }
  c->last_iterations = (uint32_t)it;
  if (r) return r;
  if (e != hipSuccess) return set_err(&c->err, CVR_ERR_HIP, "thread-bound streamingMK: %s", hipGetErrorString(e));
  return CVR_OK;
}

// The range a launch is asked for: the arguments', else the context's (cvr_set_path_range).
static void asked_range(const cvr_ctx* c, const LaunchArgs& a, uint64_t* first, uint64_t* count) {
  *first = a.range.count ? a.range.first : c->range_first;
  *count = a.range.count ? a.range.count : c->range_count;
}

LaunchPlan plan_launch(const cvr_ctx* c, const LaunchArgs& a) {
  uint64_t rf, rc;
  asked_range(c, a, &rf, &rc);
  const uint64_t f = rf < c->n_paths ? rf : c->n_paths;
  uint64_t n = c->n_paths - f;
  if (rc < n) n = rc;
  LaunchPlan plan = fill_launch(c, a, f, n, /*sharded=*/true);
  if (scheduler_for(c) != 3) return plan;
  cvr::LaunchParams& L = plan.L;
  plan.request = wpool_request(c, a.rec != nullptr, a.frame_done != nullptr);
  plan.grid = wpool_launch_grid(c, L.path_count);
  if (!c->chunk) {
    // Wave-pool dequeue chunk by the paths each wave gets: about 8 chunks per
    // wave, 64..256 paths.  Small launches (block shards of a multi-GPU render)
    // then end with the waves' last chunks evenly spread (C2 shard 1/8 on one
    // GPU: 1.09 ms at 64 vs 1.18 at 256; the whole C2 launch keeps 256).
    const uint64_t per_wave = plan.grid ? (uint64_t)L.path_count / plan.grid : 0;
    L.chunk = per_wave >= 2048 ? 256u : per_wave >= 1024 ? 128u : 64u;
  }
  L.wflags = (uint32_t)(c->drain < 0 ? 1 : c->drain) & cvr::kDrainMask;
  // samples innermost + combined splats (CVR_OPT_SAMPLE_ORDER 1): dense C2 / C3 +2.7% / +3.6%
  // (profiles/round5/ab/call6_sample_order_ab.log); C5 -1.4% before the sparse empty-region
  // mask, +2.2% with it (116.4-116.8 vs 118.9-119.7 ms, profiles/round5/ab/
  // c5_sample_order_emask.log): off by default.  The in-launch output instance
  // (cvr_render_frame) splats per lane (combining cost its dense instance two VGPR spills), and
  // per-lane splats with samples innermost put the same pixel on several lanes of one atomic
  // instruction, which the memory side serialises (C5 one render 2086 vs 2666 Msamples/s):
  // that launch always keeps the sample-major order.
  int so = c->sample_order >= 0 ? c->sample_order : 0;
  if (a.frame_done) so = 0;
  if (so == 1) L.wflags |= cvr::kUnitSampleInner | cvr::kSplatCombine;
  return plan;
}

static uint32_t spread_bits16(uint32_t v) {  // bit i -> bit 2i
  v &= 0xFFFFu;
  v = (v | (v << 8)) & 0x00FF00FFu;
  v = (v | (v << 4)) & 0x0F0F0F0Fu;
  v = (v | (v << 2)) & 0x33333333u;
  v = (v | (v << 1)) & 0x55555555u;
  return v;
}

// Order 2: within each queue's band, the launch's blocks in 2-D Morton order
// of their (x, y) in the tile, so the blocks in flight on an XCD cover a
// compact patch of the image (and so of the volume) instead of a strip of a
// block row.  C5 (4096^2, sparse cloud): 149.3 vs 155.3 ms row-major; C2
// unchanged (tools/block_order.py).  Computed on the host once per block
// layout, kept on the device.
// The table for the given tile blocks: the launch's b-th block (b in [0, L.n_blocks), split
// into the launch's XCD bands) is tile block tile_of[b]; perm[b] = the index of the block
// that takes b's turn.
static void morton_bands(const cvr::LaunchParams& L, const std::vector<uint32_t>& tile_of, std::vector<uint32_t>& perm) {
  const uint32_t nb = L.n_blocks;
  perm.resize(nb);
  std::vector<std::pair<uint32_t, uint32_t>> code(nb);
  for (uint32_t q = 0; q < L.n_queues / L.sub; ++q) {  // Morton order within each XCD band
    const uint32_t a = band_begin(L, q), e = band_begin(L, q + 1);
    for (uint32_t b = a; b < e; ++b) {
      const uint32_t tb = tile_of[b];
      const uint32_t bx = tb % L.blocks_x, by = tb / L.blocks_x;
      code[b] = {spread_bits16(bx) | (spread_bits16(by) << 1), b};
    }
    std::sort(code.begin() + a, code.begin() + e);
    for (uint32_t b = a; b < e; ++b) perm[b] = code[b].second;
  }
}

static int ensure_zorder(cvr_ctx* c, cvr::LaunchParams& L) {
  if (L.order != 1 || L.block_perm || c->order != 2 || L.n_blocks == 0) return CVR_OK;
  const uint64_t key[5] = {L.n_blocks, (uint64_t)L.n_queues / L.sub, L.blk_off, L.blk_stride, L.blocks_x};
  if (!c->d_zperm || memcmp(key, c->zkey, sizeof(key)) != 0) {
    const uint32_t nb = L.n_blocks;
    std::vector<uint32_t>& perm = c->h_zperm;
    std::vector<uint32_t> tiles(nb);  // the blocks of the shard / band
    for (uint32_t b = 0; b < nb; ++b) tiles[b] = L.blk_off + b * L.blk_stride;
    morton_bands(L, tiles, perm);
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // the previous table may still be in use
    if (c->d_zperm) (void)hipFree(c->d_zperm);
    c->d_zperm = nullptr;
    HIP_TRY(c, hipMalloc(&c->d_zperm, (size_t)nb * sizeof(uint32_t)));
    HIP_TRY(c, hipMemcpy(c->d_zperm, perm.data(), (size_t)nb * sizeof(uint32_t), hipMemcpyHostToDevice));
    memcpy(c->zkey, key, sizeof(key));
  }
  L.block_perm = c->d_zperm;
  return CVR_OK;
}

// The active block list as the launch's block table: unit_to_path takes the launch's b-th
// block as tile block block_perm[b] (blk_off 0, blk_stride 1) and needs no permutation of
// all blocks there, so a table that lists exactly the active tile blocks renders only
// them, with the path ids (and so the RNG streams) of the full launch.  Order 2 puts each
// XCD band of the list in 2-D Morton order (morton_bands), order 1 keeps it ascending.
static int ensure_active_order(cvr_ctx* c, cvr::LaunchParams& L) {
  if (!c->active_on) return CVR_OK;
  if (L.order != 1 || L.n_blocks != c->active.size() || L.blk_off != 0 || L.blk_stride != 1)
    return set_err(&c->err, CVR_ERR_STATE, "an active block list needs the pixel-block work order of whole samples");
  const uint32_t tile_blocks = L.blocks_x * (c->tile_h / 8u);
  for (uint32_t b : c->active)
    if (b >= tile_blocks) return set_err(&c->err, CVR_ERR_STATE, "active block %u outside the tile's %u", b, tile_blocks);
  c->h_active = c->active;
  if (c->order == 2 && L.n_blocks) {
    std::vector<uint32_t> perm;
    morton_bands(L, c->active, perm);
    for (uint32_t b = 0; b < L.n_blocks; ++b) c->h_active[b] = c->active[perm[b]];
  }
  if (!c->d_active || L.n_blocks == 0) return set_err(&c->err, CVR_ERR_STATE, "empty active block list");
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // the previous table may still be in use
  HIP_TRY(c, hipMemcpy(c->d_active, c->h_active.data(), (size_t)L.n_blocks * sizeof(uint32_t), hipMemcpyHostToDevice));
  L.block_perm = c->d_active;
  return CVR_OK;
}

int launch(cvr_ctx* c, const LaunchArgs& a) {
  int r = check_ready(c);
  if (r) return r;
  if (!a.out && !c->d_out) return set_err(&c->err, CVR_ERR_STATE, "no output buffer");
  if ((r = do_init(c))) return r;
  if (c->m.format != 0u) {
    // the half storage format: the wave-pool scheduler's 5-wave instances only
    const char* why = wpool_refusal(c, kForHalf);
    if (why) return set_err(&c->err, CVR_ERR_UNSUPPORTED, "the half medium format does not run with %s", why);
  }
  if (c->moments) {
    // second moments: the wave pool's two moments instances only, into the context's own buffer
    const char* why = wpool_refusal(c, kForMoments);
    if (!why && a.rec) why = "cvr_trace_launch";
    if (!why && a.frame_done) why = "cvr_render_frame's in-launch output";
    if (why) return set_err(&c->err, CVR_ERR_UNSUPPORTED, "second moments (CVR_OPT_MOMENTS 1) do not run with %s", why);
    if (c->out_owned_px < 2 * (size_t)c->tile_w * c->tile_h || c->d_out != c->d_out_owned)
      return set_err(&c->err, CVR_ERR_STATE, "the framebuffer holds no moments (cvr_set_resolution)");
  }
  if (c->have_env) {
    // an environment map: the wave pool's environment instances only
    const char* why = wpool_refusal(c, kForEnv);
    if (!why && a.rec) why = "cvr_trace_launch";
    if (!why && a.frame_done) why = "cvr_render_frame's in-launch output";
    if (why)
      return set_err(&c->err, CVR_ERR_UNSUPPORTED, "an environment map (cvr_set_environment) does not run with %s", why);
  }
  // a range as the caller gave it (count UINT64_MAX: to the end) names u32 path ids; past the
  // tile's n_paths it is clipped, past 2^32 - 1 it is a mistake
  uint64_t rf, rc;
  asked_range(c, a, &rf, &rc);
  if (rc != UINT64_MAX && (rf > 0xFFFFFFFFull || rc > 0xFFFFFFFFull || rf + rc > 0xFFFFFFFFull))
    return set_err(&c->err, CVR_ERR_INVALID, "path range [%llu, +%llu) ends past the 32-bit path ids (2^32 - 1)",
                   (unsigned long long)rf, (unsigned long long)rc);
  LaunchPlan plan = plan_launch(c, a);
  const uint64_t first = plan.first, count = plan.count;
  cvr::LaunchParams& L = plan.L;
  if ((r = ensure_active_order(c, L))) return r;
  if ((r = ensure_zorder(c, L))) return r;
  const bool eps = scatter_eps_for(c);
  // The persistent schedulers' u32 queue heads run past a queue's end by at
  // most one chunk per wave before every wave sees the queue exhausted
  // (waves: at most 4 per block of any scheduler).
  const uint64_t waves_max =
      4ull * (c->grid_override ? c->grid_override
                               : (uint64_t)std::max({c->persistent_grid, c->pool_grid, c->wpool_grid,
                                                      c->wpool_grid_sparse}));
  uint64_t units_max = L.order ? 0 : count;
  for (uint32_t q = 0; L.order && q < L.n_queues; ++q)
    units_max = std::max<uint64_t>(units_max, (uint64_t)(queue_begin(L, q + 1) - queue_begin(L, q)) * 64u * L.samples);
  if (first + count > 0xFFFFFFFFull || units_max + waves_max * L.chunk > 0xFFFFFFFFull)
    return set_err(&c->err, CVR_ERR_INVALID, "path range [%llu, +%llu) overflows the 32-bit path ids / queue heads",
                   (unsigned long long)first, (unsigned long long)count);
  HIP_TRY(c, hipMemsetAsync(c->d_work, 0, kWorkBytes, c->stream));
  HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
  c->last_iterations = 0;
  c->last_track_ms = c->last_events_ms = 0;
  if (c->rng_binding == 1) {
    if (c->kernel != CVR_KERNEL_REGENERATION_SK && c->kernel != CVR_KERNEL_STREAMING_SK &&
        c->kernel != CVR_KERNEL_SORTING_SK && c->kernel != CVR_KERNEL_STREAMING_MK)
      return set_err(&c->err, CVR_ERR_UNSUPPORTED,
                     "thread-bound RNG (CVR_OPT_RNG_BINDING 1) is regenerationSK, streamingSK, sortingSK or "
                     "streamingMK only");
    if (L.order) {  // one queue of path ids in order: the thread-bound kernels have no work bands
      L.order = 0;
      L.n_queues = 1;
    }
    if (c->kernel == CVR_KERNEL_REGENERATION_SK) {
      const uint32_t grid = c->grid_override ? c->grid_override : (uint32_t)c->cu_count * 16u;
      HIP_TRY(c, cvr::launch_regen_thread(launch_medium(c), L, eps, grid, c->stream));
    } else if (c->kernel == CVR_KERNEL_STREAMING_MK) {
      // 256-thread blocks, the occupancy grid of d_extend (RenderKernelLauncher.cu:366-392)
      const uint32_t grid = c->grid_override ? c->grid_override : (uint32_t)c->cu_count * 2u;
      if ((r = smk_thread_render(c, L, grid))) return r;
    } else {
      // StreamingVolPTsk / SortingVolPTsk: 256-thread blocks, the occupancy grid (maxOccupancyGrid,
      // RenderKernelLauncher.cu:501-508) of 2 blocks per CU unless CVR_OPT_GRID says otherwise
      const uint32_t grid = c->grid_override ? c->grid_override : (uint32_t)c->cu_count * 2u;
      HIP_TRY(c, cvr::launch_stream_thread(launch_medium(c), L, c->kernel == CVR_KERNEL_SORTING_SK, grid, c->stream));
    }
  } else if (c->kernel == CVR_KERNEL_NAIVE_MK && c->mk_compaction) {
    if ((r = mk_reference_render(c, L))) return r;
  } else if (c->kernel == CVR_KERNEL_NAIVE_MK && !mk_on_wpool(c)) {
    HIP_TRY(c, cvr::launch_naive_mk(launch_medium(c), L, c->stream));
  } else if (scheduler_for(c) == kSchedPerItem) {
    HIP_TRY(c, cvr::launch_naive(launch_medium(c), L, eps, c->stream));
  } else if (scheduler_for(c) == 0) {
    const uint32_t grid = c->grid_override ? c->grid_override : (uint32_t)c->persistent_grid;
    HIP_TRY(c, cvr::launch_persistent(launch_medium(c), L, eps, c->waves, grid, c->stream));
  } else if (scheduler_for(c) == 2) {
    const uint32_t grid = c->grid_override ? c->grid_override : (uint32_t)c->pool_grid;
    HIP_TRY(c, cvr::launch_pool(launch_medium(c), L, eps, grid, c->stream));
  } else if (scheduler_for(c) == 3) {
    const cvr::WpoolRequest& q = plan.request;
    cvr::WpoolInstance k;
    const uint32_t grid = plan.grid;
    const size_t need = cvr::wpool_select(q, &k) ? (size_t)grid * cvr::wpool_slots(k) : 0;  // (0: launch_wpool refuses)
    if (need > c->pool_T_n) {
      if (c->d_pool_T) (void)hipFree(c->d_pool_T);
      c->d_pool_T = nullptr;
      c->pool_T_n = 0;
      HIP_TRY(c, hipMalloc(&c->d_pool_T, need * sizeof(float4)));
      c->pool_T_n = need;
    }
    L.pool_T = c->d_pool_T;
    // (an environment instance has no records: the field carries the map's header instead)
    L.rec = c->have_env ? static_cast<void*>(c->d_env_hdr) : a.rec;
    if (a.frame_done) {
      // in-launch output: the first kFrameFlushers workgroups flush, the rest render
      if (L.rec || L.order != 1 || grid <= 4 * cvr::kFrameFlushers)
        return set_err(&c->err, CVR_ERR_STATE, "in-launch output needs a pixel-block launch of > %u waves",
                       4 * cvr::kFrameFlushers);
      L.frame_done = a.frame_done;
    }
    HIP_TRY(c, cvr::launch_wpool(launch_medium(c), L, q, grid, c->stream));
    // cvr_debug_last_wpool: every wave-pool launch passes here (cvr_launch_render, cvr_trace_launch's with
    // a.rec, cvr_render_frame's bands and its flushing launch with a.frame_done); an empty launch ran nothing
    if (L.path_count > 0) {
      c->last_wpool_valid = true;
      c->last_wpool = k;
      c->last_wpool_grid = grid;
    }
  } else if (L.path_count > 0) {
    if ((r = wf_render(c, L, eps))) return r;
  }
  HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
  c->timed = true;
  return CVR_OK;
}

}  // namespace cvr

extern "C" {

int cvr_launch_render(cvr_ctx* c) {
  if (!c) return cvr::set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  CVR_NOT_IN_SESSION(c, "cvr_launch_render");
  return cvr::launch(c, cvr::LaunchArgs{});
}

int cvr_launch_blocks(const cvr_ctx* c, uint32_t* n_blocks, uint32_t* n_queues, uint32_t qbeg[9]) {
  if (!c || !n_blocks || !n_queues || !qbeg) return cvr::set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  const cvr::LaunchParams L = cvr::plan_launch(c, cvr::LaunchArgs{}).L;
  *n_blocks = L.order == 1 ? L.n_blocks : 0;
  const uint32_t bands = L.n_queues / L.sub;
  *n_queues = bands;
  for (uint32_t q = 0; q < 9; ++q) qbeg[q] = q <= bands ? cvr::band_begin(L, q) : L.n_blocks;
  return CVR_OK;
}

}  // extern "C"
