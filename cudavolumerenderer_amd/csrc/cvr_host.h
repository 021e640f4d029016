// cvr_host.h - what the host sources behind the C ABI share (internal): the launch request and
// its plan (cvr_launch.cpp), and the context helpers of cvr_api.cpp that cvr_frame.cpp,
// cvr_adaptive.cpp and cvr_denoise_api.cpp call.
#pragma once
#include "cvr_ctx.h"

// (internal to the library: the C ABI's exported symbols stay what they were in one source file)
#pragma GCC visibility push(hidden)
namespace cvr {
// What a caller asks of one launch beyond the context's settings; {} is cvr_launch_render's.
struct LaunchArgs {
  float4* out = nullptr;               // the buffer to splat into (null: the context's d_out)
  void* rec = nullptr;                 // cvr_trace_launch: the launch's records
  unsigned int* frame_done = nullptr;  // cvr_render_frame's in-launch output: the per-block counts
  struct { uint32_t first = 0, count = 0; } band;   // cvr_render_frame's band of tile blocks (count 0: every block)
  struct { uint64_t first = 0, count = 0; } range;  // the path range, in place of the context's (count 0: the context's)
};

// What a launch of the context with these arguments is, decided in one place (plan_launch).
struct LaunchPlan {
  uint64_t first = 0, count = 0;  // the range, clipped to the tile's n_paths (before any sharding)
  LaunchParams L{};               // (block_perm, pool_T, rec and frame_done are the launch's to set)
  bool block_order = false;       // the scheduler takes work units (unit_to_path), this launch's in pixel-block order
  uint32_t grid = 0;              // wave pool: the grid in waves (other schedulers: 0)
  WpoolRequest request{};         // wave pool: what the launch asks of k_wpool
};
LaunchPlan plan_launch(const cvr_ctx* c, const LaunchArgs& a);
// The parameters of the per-path traces: paths [first, first + count) as given, not clipped and not sharded.
LaunchParams trace_params(const cvr_ctx* c, uint32_t first, uint32_t count);
// One render launch on the context's stream (cvr_launch_render without the session guard).
int launch(cvr_ctx* c, const LaunchArgs& a);

// Scheduler policy (cvr_launch.cpp)
constexpr int kSchedPerItem = 4;
int scheduler_for(const cvr_ctx* c);
bool scatter_eps_for(const cvr_ctx* c);
MediumParams launch_medium(const cvr_ctx* c);
enum : unsigned { kForHalf = 1, kForMoments = 2, kForEnv = 4, kForAll = 7 };
const char* wpool_refusal(const cvr_ctx* c, unsigned feature);
FastDiv make_fastdiv(uint32_t d);
int do_init(cvr_ctx* c);

// Context helpers (cvr_api.cpp)
int ensure_output(cvr_ctx* c);
int check_ready(cvr_ctx* c);
uint32_t seed_after_resets(const cvr_ctx* c, uint32_t seed, uint32_t resets);
// CVR_ERR_INVALID unless a host image of host_floats floats holds the w x h rgba pixels of `what`
int check_host_floats(cvr_ctx* c, size_t host_floats, uint32_t w, uint32_t h, const char* what);
// acc += s: the eight counters, and of words and kernel_ms those named in `fields`
enum : unsigned { kStatWords = 1, kStatKernelMs = 2 };
void add_stats(cvr_stats& acc, const cvr_stats& s, unsigned fields);
}  // namespace cvr
#pragma GCC visibility pop
