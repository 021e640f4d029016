// cvr_frame.cpp - the renderers of the C ABI over the launch: CudaVolPath's tile loop
// (cvr_render_image / cvr_render_tiles), one device's share of a multi-device render, and
// cvr_render_frame with its bands on helper contexts and its in-launch output (the flusher waves:
// cvr_wpool.hip; the tile and block transfers: cvr_kernels.hip).
//
// Reference map:
//   CudaVolPath::render / runIterations / getImage / prepareForNextIterations
//                                                CudaVolPath.cpp:189-347
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "cvr_host.h"

using cvr::check_ready;
using cvr::do_init;
using cvr::ensure_device;
using cvr::ensure_output;
using cvr::seed_after_resets;
using cvr::set_err;

extern "C" {

// ------------------------------------------------------------ renderer ----
int cvr_render_image(cvr_ctx* c, const cvr_render_desc* d, void* device_image, float* host_image, cvr_stats* stats) {
  return cvr_render_tiles(c, d, 0, 1, device_image, host_image, stats);
}

int cvr_render_tiles(cvr_ctx* c, const cvr_render_desc* d, uint32_t first_tile, uint32_t tile_stride,
                     void* device_image, float* host_image, cvr_stats* stats) {
  if (!c || !d) return set_err(c ? &c->err : nullptr, CVR_ERR_INVALID, "NULL argument");
  CVR_NOT_IN_SESSION(c, "cvr_render_image / cvr_render_tiles");
  if (c->moments)
    return set_err(&c->err, CVR_ERR_UNSUPPORTED,
                   "second moments (CVR_OPT_MOMENTS 1) do not run with cvr_render_image / cvr_render_tiles");
  if (tile_stride == 0) return set_err(&c->err, CVR_ERR_INVALID, "tile stride 0");
  uint32_t tile_dim[2];
  int r = cvr_tiling(d->resolution[0], d->resolution[1], d->n_tiles[0], d->n_tiles[1], tile_dim);
  if (r) return set_err(&c->err, r, "%s", cvr_last_error(nullptr));
  if ((r = cvr_set_resolution(c, tile_dim[0], tile_dim[1]))) return r;
  if ((r = cvr_set_iterations(c, d->iterations))) return r;  // setNIterations
  if ((r = check_ready(c))) return r;
  const uint32_t W = d->resolution[0], H = d->resolution[1];
  const uint32_t ntiles = d->n_tiles[0] * d->n_tiles[1];
  if (ntiles == 1 && first_tile == 0 && !device_image && host_image && !c->external_out) {
    // one tile into host memory: cvr_render_frame (no scratch image per call; the same
    // clear, launch, Scale + copy and seed advance as the loop below)
    if ((r = cvr_set_offset(c, 0, 0))) return r;
    if ((r = ensure_output(c))) return r;
    return cvr_render_frame(c, host_image, (size_t)W * H * 4u, 1, stats);
  }
  float4* dimg = static_cast<float4*>(device_image);
  float4* tmp_img = nullptr;
  if (!dimg && host_image) {
    HIP_TRY(c, hipMalloc(&tmp_img, (size_t)W * H * sizeof(float4)));
    const hipError_t e = hipMemsetAsync(tmp_img, 0, (size_t)W * H * sizeof(float4), c->stream);
    if (e != hipSuccess) {
      (void)hipFree(tmp_img);
      return set_err(&c->err, CVR_ERR_HIP, "image buffer: %s", hipGetErrorString(e));
    }
    dimg = tmp_img;
  }
  const uint32_t seed0 = c->seed;
  cvr_stats acc{};
  // initRenderState: memset the accumulator
  if ((r = cvr_clear_output(c))) goto done;
  for (uint32_t k = first_tile; k < ntiles; k += tile_stride) {
    // the seed tile k has in the sequential tile loop (k resets after seed0)
    c->seed = seed_after_resets(c, seed0, k);
    uint32_t org[2];
    cvr_tile_origin(k, d->n_tiles[0], tile_dim, org);
    if ((r = cvr_set_offset(c, org[0], org[1]))) goto done;  // copyOffset
    if ((r = cvr_launch_render(c))) goto done;               // launchRender
    if (dimg) {  // getImage: scale by 1/current_iteration_ into the image
      hipError_t e = cvr::launch_tile_to_image(c->d_out, tile_dim[0], tile_dim[1], dimg, W, org[0], org[1],
                                               (float)d->iterations, c->stream);
      if (e != hipSuccess) {
        r = set_err(&c->err, CVR_ERR_HIP, "tile transfer: %s", hipGetErrorString(e));
        goto done;
      }
    }
    cvr_stats s{};
    if ((r = cvr_get_stats(c, &s))) goto done;  // synchronises (reset() does too)
    cvr::add_stats(acc, s, cvr::kStatWords | cvr::kStatKernelMs);
    if ((r = cvr_reset(c))) goto done;  // prepareForNextIterations
    if (ntiles != 1 && (r = cvr_clear_output(c))) goto done;
  }
  c->seed = seed_after_resets(c, seed0, ntiles);  // as after the whole tile loop
  if (host_image) {
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(host_image, dimg, (size_t)W * H * sizeof(float4), hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
      r = set_err(&c->err, CVR_ERR_HIP, "image copy: %s", hipGetErrorString(e));
      goto done;
    }
  }
  if (stats) *stats = acc;
done:
  if (tmp_img) {
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(tmp_img);
  }
  return r;
}

// One device's share of a multi-device render (cvr --devices):
// its tiles of the tile loop (tile k -> device k mod N, CudaVolPath.cpp:249-280
// split over devices) or its block shard of the one tile, normalised and stored
// by a kernel straight into the shared pinned host image at their places.  The
// shares are pixel-disjoint, so N of these calls (one host thread per device)
// leave cvr_render_image's image in the one host buffer: no reduction.
int cvr_render_share_to_host(cvr_ctx* c, const cvr_render_desc* d, uint32_t first_tile, uint32_t tile_stride,
                             float* host_image, size_t host_floats, cvr_stats* stats) {
  if (!c || !d || !host_image) return set_err(c ? &c->err : nullptr, CVR_ERR_INVALID, "NULL argument");
  CVR_NOT_IN_SESSION(c, "cvr_render_share_to_host");
  if (c->moments)
    return set_err(&c->err, CVR_ERR_UNSUPPORTED,
                   "second moments (CVR_OPT_MOMENTS 1) do not run with cvr_render_share_to_host");
  if (tile_stride == 0) return set_err(&c->err, CVR_ERR_INVALID, "tile stride 0");
  const uint32_t W = d->resolution[0], H = d->resolution[1];
  int r = cvr::check_host_floats(c, host_floats, W, H, "image");
  if (r) return r;
  if ((uintptr_t)host_image & 15u) return set_err(&c->err, CVR_ERR_INVALID, "host image must be 16-byte aligned");
  if ((r = ensure_device(c))) return r;
  void* dhost = nullptr;  // the host image's device address (pinned / registered memory)
  hipError_t e = hipHostGetDevicePointer(&dhost, host_image, 0);
  if (e != hipSuccess || !dhost) {
    (void)hipGetLastError();
    return set_err(&c->err, CVR_ERR_INVALID, "host image is not pinned or registered (cvr_host_alloc)");
  }
  const uint32_t ntiles = d->n_tiles[0] * d->n_tiles[1];
  if (ntiles != 1 || c->shard_world == 1) {
    // tiles k = first_tile, first_tile + stride, ...: each tile's pixels only (k_tile_to_image
    // into the mapped host image), each tile with its sequential-loop seed
    if (ntiles != 1 && c->shard_world != 1)
      return set_err(&c->err, CVR_ERR_INVALID, "a tile share and a block shard at once");
    return cvr_render_tiles(c, d, first_tile, tile_stride, dhost, nullptr, stats);
  }
  // one tile, this context's block shard: launch, then its 8x8 blocks into the host image
  if (first_tile != 0) return set_err(&c->err, CVR_ERR_INVALID, "one tile: the share is the block shard");
  if (W % 8 || H % 8) return set_err(&c->err, CVR_ERR_INVALID, "block shards need sides that are multiples of 8");
  if ((r = cvr_set_resolution(c, W, H)) || (r = cvr_set_iterations(c, d->iterations)) || (r = cvr_set_offset(c, 0, 0)))
    return r;
  if ((r = check_ready(c)) || (r = ensure_output(c))) return r;
  // the launch must really be this context's 8x8-block shard: the plan falls back to a
  // contiguous slice of path ids (part-sums of other pixels) without the block work order
  // (thread-bound RNG, CVR_OPT_ORDER 0, the per-item / wavefront schedulers, > 2^20 samples)
  if (c->shard_world > 1 && !cvr::plan_launch(c, cvr::LaunchArgs{}).block_order)
    return set_err(&c->err, CVR_ERR_UNSUPPORTED,
                   "this launch has no 8x8-block work order (thread-bound RNG, CVR_OPT_ORDER 0, a per-item or "
                   "wavefront scheduler, or more than 2^20 samples), so it cannot be block-sharded over devices");
  if ((r = cvr_clear_output(c)) || (r = cvr_launch_render(c))) return r;
  e = cvr::launch_blocks_to_host(reinterpret_cast<const float*>(c->d_out), static_cast<float*>(dhost), W, H,
                                 c->shard_rank, c->shard_world, (float)d->iterations, c->stream);
  if (e != hipSuccess) return set_err(&c->err, CVR_ERR_HIP, "blocks to host: %s", hipGetErrorString(e));
  cvr_stats s{};
  if ((r = cvr_get_stats(c, &s))) return r;  // synchronises: the blocks are in the host image
  if (stats) *stats = s;
  return cvr_reset(c);  // prepareForNextIterations
}

// The launcher settings a helper context of cvr_render_frame takes from its
// parent: everything but its own resources (stream, work queues, scratch).
static void copy_settings(cvr_ctx* d, const cvr_ctx* s) { static_cast<cvr::Settings&>(*d) = *s; }

// cvr_render_frame with the in-launch output: the clear, the header and the block
// counts, one launch whose flusher waves store the normalised blocks into the host
// image (device address dhost), and the copy after the launch only if a flusher gave up.
static int render_frame_flush(cvr_ctx* c, void* dhost, cvr_stats* stats) {
  const uint32_t W = c->tile_w, H = c->tile_h;
  const size_t px = (size_t)W * H, nb = (size_t)(W / 8u) * (H / 8u);
  if (c->flush_blocks < nb) {
    if (c->d_flush) (void)hipFree(c->d_flush);
    c->d_flush = nullptr;
    c->flush_blocks = 0;
    HIP_TRY(c, hipMalloc(&c->d_flush, sizeof(cvr::FrameFlush) + nb * cvr::kDoneStride * sizeof(unsigned int)));
    c->flush_blocks = nb;
    c->flush_hdr_valid = false;
  }
  if (!c->h_flush_status) {
    HIP_TRY(c, hipHostMalloc(&c->h_flush_status, 64, hipHostMallocDefault));
  }
  if (!c->frame_ev[0])
    for (auto& e : c->frame_ev) HIP_TRY(c, hipEventCreate(&e));
  unsigned int* dstatus = nullptr;
  HIP_TRY(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&dstatus), c->h_flush_status, 0));
  memset(c->h_flush_status, 0, 64);  // the previous frame has ended (its call synchronised)
  cvr::FrameFlush hdr{};
  hdr.host = static_cast<float4*>(dhost);
  hdr.status = dstatus;
  hdr.host_w = W;
  hdr.scale = (float)c->iterations;
  hdr.give_up = c->frame_flush == 2 ? 1u : 0u;
  // the header only travels when it changed (the same host image frame after frame: none)
  const bool send_hdr = !c->flush_hdr_valid || memcmp(&hdr, &c->flush_hdr, sizeof(hdr)) != 0;
  c->flush_hdr = hdr;
  unsigned int* done = reinterpret_cast<unsigned int*>(c->d_flush + sizeof(cvr::FrameFlush));
  HIP_TRY(c, hipMemsetAsync(c->d_out, 0, px * sizeof(float4), c->stream));  // initRenderState
  if (send_hdr) {
    c->flush_hdr_valid = false;
    HIP_TRY(c, hipMemcpyAsync(c->d_flush, &c->flush_hdr, sizeof(cvr::FrameFlush), hipMemcpyHostToDevice, c->stream));
    c->flush_hdr_valid = true;
  }
  HIP_TRY(c, hipMemsetAsync(done, 0, nb * cvr::kDoneStride * sizeof(unsigned int), c->stream));
  HIP_TRY(c, hipEventRecord(c->frame_ev[0], c->stream));
  cvr::LaunchArgs args;
  args.frame_done = done;
  int r = cvr::launch(c, args);
  if (r) return r;
  HIP_TRY(c, hipEventRecord(c->frame_ev[1], c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  uint64_t stored = 0;
  for (uint32_t f = 0; f < cvr::kFrameFlushers; ++f) stored += c->h_flush_status[f];
  if (c->h_flush_status[cvr::kFrameFlushers] != 0 || stored != nb) {
    // a flusher gave up: getImage the usual way (the framebuffer is complete)
    ++c->flush_fallbacks;
    c->flush_last_blocks = 0;
    HIP_TRY(c, cvr::launch_image_to_host(reinterpret_cast<const float*>(c->d_out), static_cast<float*>(dhost),
                                         px * 4, (float)c->iterations, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  } else {
    c->flush_last_blocks = (uint32_t)stored;
  }
  c->seed = seed_after_resets(c, c->seed, 1);  // reset(): prepareForNextIterations
  if (!stats) return CVR_OK;
  cvr_stats acc{};
  if ((r = cvr_get_stats(c, &acc))) return r;
  float ms = 0.f;  // clear to the end of the launch
  HIP_TRY(c, hipEventElapsedTime(&ms, c->frame_ev[0], c->frame_ev[1]));
  acc.kernel_ms = ms;
  c->last = acc;
  *stats = acc;
  return CVR_OK;
}

int cvr_frame_flush_info(const cvr_ctx* c, uint32_t* blocks, uint32_t* fallbacks) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL ctx");
  if (blocks) *blocks = c->flush_last_blocks;
  if (fallbacks) *fallbacks = c->flush_fallbacks;
  return CVR_OK;
}

int cvr_render_frame(cvr_ctx* c, float* host_image, size_t host_floats, uint32_t parts, cvr_stats* stats) {
  if (!c || !host_image) return set_err(c ? &c->err : nullptr, CVR_ERR_INVALID, "NULL argument");
  CVR_NOT_IN_SESSION(c, "cvr_render_frame");
  if (c->moments)
    return set_err(&c->err, CVR_ERR_UNSUPPORTED, "second moments (CVR_OPT_MOMENTS 1) do not run with cvr_render_frame");
  int r = check_ready(c);
  if (r) return r;
  if ((r = cvr::check_host_floats(c, host_floats, c->tile_w, c->tile_h, "tile"))) return r;
  if (!c->d_out) return set_err(&c->err, CVR_ERR_STATE, "no output buffer");
  if ((r = do_init(c))) return r;
  const uint32_t W = c->tile_w, H = c->tile_h;
  const size_t px = (size_t)W * H;
  // bands need the pixel-block work order of a whole-sample, unsharded, queued launch
  const cvr::LaunchPlan plan = cvr::plan_launch(c, cvr::LaunchArgs{});
  const uint32_t brows = (plan.block_order && c->shard_world == 1) ? H / 8u : 0u;
  if (parts == 0) parts = 1;
  if (c->have_env) parts = 1;  // the environment is the context's own: no helper contexts (and no in-launch output)
  parts = std::min<uint32_t>(parts, 3u);
  if (brows < parts) parts = brows ? brows : 1u;
  // band k takes (parts - k) shares of the block rows: the last band, whose copy
  // the frame waits for, is the smallest
  uint32_t row0[4] = {0, 0, 0, 0};
  {
    const uint32_t shares = parts * (parts + 1) / 2;
    uint32_t acc = 0;
    for (uint32_t k = 0; k < parts; ++k) {
      acc += parts - k;
      row0[k + 1] = k + 1 == parts ? brows : (uint32_t)((uint64_t)brows * acc / shares);
    }
  }
  // in-launch output (CVR_OPT_FRAME_FLUSH): one part on the wave pool, an instance with that
  // output for the launch, and a host image the GPU can store into
  void* dhost = nullptr;
  cvr::WpoolRequest flushing = plan.request;
  flushing.flush = true;
  cvr::WpoolInstance inst;
  if (c->frame_flush && parts == 1 && brows && cvr::scheduler_for(c) == 3 && cvr::wpool_select(flushing, &inst) &&
      plan.grid > 4 * cvr::kFrameFlushers) {
    if (hipHostGetDevicePointer(&dhost, host_image, 0) != hipSuccess) {
      (void)hipGetLastError();  // pageable memory: not an error, the copy path below
      dhost = nullptr;
    }
  }
  if (dhost) return render_frame_flush(c, dhost, stats);
  c->flush_last_blocks = 0;
  while (c->frame_kids.size() + 1 < parts) {
    cvr_ctx* k = nullptr;
    if ((r = cvr_create(c->device, c->kernel, &k)))
      return set_err(&c->err, r, "frame helper: %s", cvr_last_error(nullptr));
    c->frame_kids.push_back(k);
  }
  if (!c->frame_copy) {
    int lo = 0, hi = 0;
    HIP_TRY(c, hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIP_TRY(c, hipStreamCreateWithPriority(&c->frame_copy, hipStreamNonBlocking, hi));
  }
  // the same events as render_frame_flush's (created once, whichever path comes first)
  if (!c->frame_ev[0])
    for (auto& e : c->frame_ev) HIP_TRY(c, hipEventCreate(&e));
  if (c->frame_px < px) {
    HIP_TRY(c, hipStreamSynchronize(c->frame_copy));
    if (c->d_frame) (void)hipFree(c->d_frame);
    c->d_frame = nullptr;
    c->frame_px = 0;
    HIP_TRY(c, hipMalloc(&c->d_frame, px * sizeof(float4)));
    c->frame_px = px;
  }
  // clear (initRenderState), then every band on its own stream
  HIP_TRY(c, hipMemsetAsync(c->d_out, 0, px * sizeof(float4), c->stream));
  HIP_TRY(c, hipEventRecord(c->frame_ev[0], c->stream));
  cvr_ctx* who[3] = {c, nullptr, nullptr};
  for (uint32_t k = 1; k < parts; ++k) {
    cvr_ctx* kid = c->frame_kids[k - 1];
    copy_settings(kid, c);
    if ((r = do_init(kid))) return set_err(&c->err, r, "frame helper: %s", kid->err.c_str());
    HIP_TRY(c, hipStreamWaitEvent(kid->stream, c->frame_ev[0], 0));
    who[k] = kid;
  }
  const float scale = (float)c->iterations;
  for (uint32_t k = 0; k < parts; ++k) {
    cvr_ctx* x = who[k];
    cvr::LaunchArgs args;
    args.out = c->d_out;  // the helpers splat into the parent's framebuffer
    args.band.first = brows ? row0[k] * (W / 8u) : 0u;
    args.band.count = brows ? (row0[k + 1] - row0[k]) * (W / 8u) : 0u;
    r = cvr::launch(x, args);
    if (r) return x == c ? r : set_err(&c->err, r, "frame band %u: %s", k, x->err.c_str());
    HIP_TRY(c, hipEventRecord(c->frame_ev[1 + k], x->stream));
    // getImage of the band's rows (ImageBufferTransfer.cu:61-78: Scale, then the D->H
    // copy) on the copy stream, while the later bands render
    const uint32_t y0 = brows ? row0[k] * 8u : 0u, y1 = brows ? row0[k + 1] * 8u : H;
    HIP_TRY(c, hipStreamWaitEvent(c->frame_copy, c->frame_ev[1 + k], 0));
    HIP_TRY(c, cvr::launch_tile_to_image(c->d_out + (size_t)y0 * W, W, y1 - y0, c->d_frame, W, 0, y0, scale,
                                         c->frame_copy));
    HIP_TRY(c, hipMemcpyAsync(host_image + (size_t)y0 * W * 4, c->d_frame + (size_t)y0 * W,
                              (size_t)(y1 - y0) * W * sizeof(float4), hipMemcpyDeviceToHost, c->frame_copy));
  }
  HIP_TRY(c, hipStreamSynchronize(c->frame_copy));
  c->seed = seed_after_resets(c, c->seed, 1);  // reset(): prepareForNextIterations
  if (!stats) return CVR_OK;  // the counters cost a synchronous read per band
  cvr_stats acc{};
  for (uint32_t k = 0; k < parts; ++k) {
    cvr_stats s{};
    if ((r = cvr_get_stats(who[k], &s))) return who[k] == c ? r : set_err(&c->err, r, "%s", who[k]->err.c_str());
    cvr::add_stats(acc, s, cvr::kStatWords);
  }
  float ms = 0.f;  // clear to the end of the band that ends last
  for (uint32_t k = 0; k < parts; ++k) {
    float t = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&t, c->frame_ev[0], c->frame_ev[1 + k]));
    ms = std::max(ms, t);
  }
  acc.kernel_ms = ms;
  c->last = acc;
  *stats = acc;
  return CVR_OK;
}
}  // extern "C"
