// cvr_project.hip - the field projections on the device (cvr_field_project*, include/cvr.h).  The
// arithmetic is project_pixel of cvr_project.h, the definition cvr_field_project_host runs on the
// CPU: this kernel only maps pixels onto lanes and taps onto loads of the caller's field, so
// device and host agree bit for bit.
//
// k_features' mapping: one lane per pixel, a wave per 8x8 pixel block (neighbouring rays march
// through neighbouring voxels, so the taps of a wave fall into few cache lines), a 256-thread
// workgroup 2x2 such blocks, the workgroups row-major over a 1-D grid of ceil(w / 16) *
// ceil(h / 16).  Lanes outside the tile leave at once; chords differ and the isosurface ends a
// march at its hit, so the loop runs under the exec mask to the wave's last live lane, and the
// refinement and the gradient's six lookups run once per lane after it.  The eight taps of a
// lookup are eight plain loads of one element each: the field is aligned to its element only (a
// tensor view may start anywhere in its allocation), and an x pair straddles a row's end where
// the clamp folds it, so no wider load is right for every pair.  Nothing is collective: no LDS, no
// barrier, no atomics, no waits on other waves; the march is bounded by max_steps, the refinement
// by refine <= 8, the specular's squarings by shininess_log2 <= 10.  One instance per scalar type
// and mode.
#include "cvr_project.h"
#include "cvr_walk.h"

namespace cvr {
namespace {

template <class T, int Mode>
__global__ __launch_bounds__(256) void k_project(const T* __restrict__ scalar, const ProjectParams R,
                                                 float4* __restrict__ out_rgba, float* __restrict__ out_value,
                                                 float* __restrict__ out_depth) {
  const FeatureParams& P = R.Q.F;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t groups_x = (P.tile_w + 15u) >> 4;
  const uint32_t gy = blockIdx.x / groups_x, gx = blockIdx.x - gy * groups_x;
  const uint32_t ix = gx * 16u + (wave & 1u) * 8u + (lane & 7u), iy = gy * 16u + (wave >> 1) * 8u + (lane >> 3);
  if (ix >= P.tile_w || iy >= P.tile_h) return;
  const ProjectOut f = project_pixel<ProjectTexels<T>, Mode>(ProjectTexels<T>{scalar, P.res[0], P.res[1]}, R, ix, iy);
  const size_t i = (size_t)iy * P.tile_w + ix;
  gstore4(out_rgba + i, make_float4(f.r, f.g, f.b, f.a));
  if (out_value) out_value[i] = f.value;
  if (out_depth) out_depth[i] = f.depth;
}

template <class T>
void launch_typed(const void* scalar, int mode, uint32_t grid, const ProjectParams& R, float4* out_rgba, float* out_value,
                  float* out_depth, hipStream_t s) {
  const T* f = static_cast<const T*>(scalar);
  switch (mode) {
    case kProjectMax:
      hipLaunchKernelGGL((k_project<T, kProjectMax>), dim3(grid), dim3(256), 0, s, f, R, out_rgba, out_value, out_depth);
      break;
    case kProjectMin:
      hipLaunchKernelGGL((k_project<T, kProjectMin>), dim3(grid), dim3(256), 0, s, f, R, out_rgba, out_value, out_depth);
      break;
    case kProjectMean:
      hipLaunchKernelGGL((k_project<T, kProjectMean>), dim3(grid), dim3(256), 0, s, f, R, out_rgba, out_value, out_depth);
      break;
    default:
      hipLaunchKernelGGL((k_project<T, kProjectIso>), dim3(grid), dim3(256), 0, s, f, R, out_rgba, out_value, out_depth);
      break;
  }
}

}  // namespace

hipError_t launch_project(const void* scalar, uint32_t scalar_type, int mode, const ProjectParams& R, float4* out_rgba,
                          float* out_value, float* out_depth, hipStream_t s) {
  const FeatureParams& P = R.Q.F;
  const uint64_t voxels = (uint64_t)P.res[0] * P.res[1] * P.res[2];  // (each factor pair checked by the caller)
  if (!scalar || !out_rgba || P.tile_w == 0 || P.tile_h == 0 || (uint64_t)P.tile_w * P.tile_h > (1ull << 24) ||
      P.max_steps == 0 || P.max_steps > 65536u || R.Q.shininess_log2 > 10u || R.refine > 8u || voxels == 0 ||
      voxels > 0xFFFFFFFFull || scalar_type > 3u || mode < kProjectMax || mode > kProjectIso)
    return hipErrorInvalidValue;
  const uint32_t grid = ((P.tile_w + 15u) >> 4) * ((P.tile_h + 15u) >> 4);
  switch (scalar_type) {
    case 1: launch_typed<uint8_t>(scalar, mode, grid, R, out_rgba, out_value, out_depth, s); break;
    case 2: launch_typed<uint16_t>(scalar, mode, grid, R, out_rgba, out_value, out_depth, s); break;
    case 3: launch_typed<int16_t>(scalar, mode, grid, R, out_rgba, out_value, out_depth, s); break;
    default: launch_typed<float>(scalar, mode, grid, R, out_rgba, out_value, out_depth, s); break;
  }
  return hipGetLastError();
}

}  // namespace cvr
