// cvr_gradient.h - a voxel's central-difference gradient magnitude, once: the per-voxel formula, the
// single-voxel stencil, the host statements' loop over a field and the device kernels' walk over
// one.  The 2-D transfer functions (cvr_classify_gradient_host, k_gradient), the leaf kernels'
// voxel source and the field statistics and histograms (cvr_field_*_host, k_field_walk) all compile
// these definitions, so host statement and kernel return the same bits.  fp32 only, every
// operation in the written order (-ffp-contract=off, correctly rounded / and sqrt).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cvr {

// (s - lo) / (hi - lo) clamped to [0, 1]: the classifications' u and v and the histograms'
// coordinates.  A NaN gives 0.
__host__ __device__ inline float unit_clamp(float s, float lo, float hi) {
  const float t = (s - lo) / (hi - lo);
  float u = t > 0.0f ? t : 0.0f;  // a NaN compares false: 0
  u = u < 1.0f ? u : 1.0f;
  return u;
}

// Per axis x, y, z: 1.0f / spacing and 0.5f / spacing, rounded once on the host (gradient_axes)
struct GradientAxes {
  float h1[3] = {1.0f, 1.0f, 1.0f}, h2[3] = {0.5f, 0.5f, 0.5f};
};
inline GradientAxes gradient_axes(const float spacing[3]) {
  GradientAxes a;
  for (int k = 0; k < 3; ++k) {
    a.h1[k] = 1.0f / spacing[k];
    a.h2[k] = 0.5f / spacing[k];
  }
  return a;
}

// Gradient-magnitude transfer functions (cvr_set_medium_gradient, cvr_classify_gradient_host).
// The 2-D classification cvr.h states.  table: m rows of n entries.
struct GradientParams {
  uint32_t n, m;  // entries per row (scalar axis), rows (gradient axis)
  float lo, hi, glo, ghi;
  GradientAxes axes;
};
// The lower and upper neighbour of coordinate c on an axis of n voxels, and the factor of their
// difference: the central one when both exist, else the one-sided one.
__host__ __device__ inline void gradient_neighbours(uint32_t c, uint32_t n, float h1, float h2, uint32_t& cm,
                                                    uint32_t& cp, float& k) {
  cm = c > 0u ? c - 1u : c;
  cp = c + 1u < n ? c + 1u : c;
  k = cp - cm == 2u ? h2 : h1;
}
__host__ __device__ inline float gradient_magnitude(float sxm, float sxp, float kx, float sym, float syp, float ky,
                                                    float szm, float szp, float kz) {
  const float gx = (sxp - sxm) * kx, gy = (syp - sym) * ky, gz = (szp - szm) * kz;
  const float q = (gx * gx + gy * gy) + gz * gz;
  return __builtin_sqrtf(q);
}
// s: the voxel; mag: its gradient magnitude.  Returns (r, g, b, density).
__host__ __device__ inline float4 gradient_classify(float s, float mag, const float4* table, const GradientParams& p) {
  const float u = unit_clamp(s, p.lo, p.hi), v = unit_clamp(mag, p.glo, p.ghi);
  const float xt = u * (float)(p.n - 1u), yt = v * (float)(p.m - 1u);
  const uint32_t ci = (uint32_t)__builtin_floorf(xt), i = ci < p.n - 2u ? ci : p.n - 2u;
  const uint32_t cj = (uint32_t)__builtin_floorf(yt), j = cj < p.m - 2u ? cj : p.m - 2u;
  const float f = xt - (float)i, h = yt - (float)j;
  const float4 P = table[j * p.n + i], Q = table[j * p.n + i + 1u];
  const float4 R = table[(j + 1u) * p.n + i], W = table[(j + 1u) * p.n + i + 1u];
  float4 a, b, e;
  a.x = P.x + f * (Q.x - P.x), a.y = P.y + f * (Q.y - P.y), a.z = P.z + f * (Q.z - P.z), a.w = P.w + f * (Q.w - P.w);
  b.x = R.x + f * (W.x - R.x), b.y = R.y + f * (W.y - R.y), b.z = R.z + f * (W.z - R.z), b.w = R.w + f * (W.w - R.w);
  e.x = a.x + h * (b.x - a.x), e.y = a.y + h * (b.y - a.y), e.z = a.z + h * (b.z - a.z), e.w = a.w + h * (b.w - a.w);
  return e;
}

// The gradient magnitude of voxel (x, y, z) of a field of res voxels, x fastest: the voxel's up to
// six in-grid neighbours through read(index) -> float, wherever the field lies.
template <class Read>
__host__ __device__ inline float gradient_at(Read&& read, uint32_t x, uint32_t y, uint32_t z, const uint32_t res[3],
                                             const GradientAxes& a) {
  const uint32_t nx = res[0], ny = res[1];
  uint32_t xm, xp, ym, yp, zm, zp;
  float kx, ky, kz;
  gradient_neighbours(x, nx, a.h1[0], a.h2[0], xm, xp, kx);
  gradient_neighbours(y, ny, a.h1[1], a.h2[1], ym, yp, ky);
  gradient_neighbours(z, res[2], a.h1[2], a.h2[2], zm, zp, kz);
  const size_t row = ((size_t)z * ny + y) * nx;
  const float sxm = read(row + xm), sxp = read(row + xp);
  const float sym = read(((size_t)z * ny + ym) * nx + x), syp = read(((size_t)z * ny + yp) * nx + x);
  const float szm = read(((size_t)zm * ny + y) * nx + x), szp = read(((size_t)zp * ny + y) * nx + x);
  return gradient_magnitude(sxm, sxp, kx, sym, syp, ky, szm, szp, kz);
}

// The host statements' loop: fn(i, s, mag) for every voxel i of a field in host memory, x
// fastest, with its value and its gradient magnitude; the row offsets are hoisted out of the x loop.
template <class Read, class F>
inline void gradient_for_each(Read&& read, const uint32_t res[3], const GradientAxes& a, F&& fn) {
  const uint32_t nx = res[0], ny = res[1], nz = res[2];
  for (uint32_t z = 0; z < nz; ++z) {
    uint32_t zm, zp;
    float kz;
    gradient_neighbours(z, nz, a.h1[2], a.h2[2], zm, zp, kz);
    for (uint32_t y = 0; y < ny; ++y) {
      uint32_t ym, yp;
      float ky;
      gradient_neighbours(y, ny, a.h1[1], a.h2[1], ym, yp, ky);
      const size_t row = ((size_t)z * ny + y) * nx, rym = ((size_t)z * ny + ym) * nx, ryp = ((size_t)z * ny + yp) * nx,
                   rzm = ((size_t)zm * ny + y) * nx, rzp = ((size_t)zp * ny + y) * nx;
      for (uint32_t x = 0; x < nx; ++x) {
        uint32_t xm, xp;
        float kx;
        gradient_neighbours(x, nx, a.h1[0], a.h2[0], xm, xp, kx);
        fn(row + x, read(row + x),
           gradient_magnitude(read(row + xm), read(row + xp), kx, read(rym + x), read(ryp + x), ky, read(rzm + x),
                              read(rzp + x), kz));
      }
    }
  }
}

// The device walk's geometry (cvr_debug_build_geometry and cvr_debug_field_geometry report it): a
// task is 256 consecutive x of one y over kWalkZ consecutive z.
constexpr uint32_t kWalkTaskCap = 4096;  // the walk's grid: tasks beyond it are a workgroup's next trip
constexpr uint32_t kWalkZ = 16;          // z planes per task
__host__ __device__ inline size_t gradient_walk_tasks(uint32_t nx, uint32_t ny, uint32_t nz) {
  return (size_t)((nx + 255u) / 256u) * ny * ((nz + kWalkZ - 1u) / kWalkZ);
}

// The device walk: fn(in, x, y, z, cur, mag) for every voxel of the field S, called by every lane
// of a workgroup of 256 (in false: the lane lies past the row's end, and cur and mag are those of
// the row's last voxel; fn may use the whole wave).  A work-item keeps its voxel's z - 1, z, z + 1
// in registers while it marches along z, so the z neighbours cost one load per voxel and step.
// The x neighbours come from the adjacent lanes (a load only in a wave's first and last lane), the
// y neighbours are two loads of rows that the tasks of y - 1 and y + 1 read as their own (cache
// hits, not memory traffic, when those tasks run close in time on one XCD: consecutive tasks are
// consecutive x-runs, then consecutive y).  A wave's loads of a step are 64 consecutive voxels.
// The grid is at most kWalkTaskCap workgroups, a multiple of 8 where there are 8.
// skip(xb, x0, y, z0, z1), asked by every lane once per task before anything is read: true leaves
// the task out (its voxels are x in [xb, xb + 256) of row y over z in [z0, z1); x0 is the lane's
// x, which may lie past the row).  Its answer must be the workgroup's.
template <class T, class F, class Skip>
__device__ __forceinline__ void gradient_walk(const T* __restrict__ S, uint32_t nx, uint32_t ny, uint32_t nz,
                                              const GradientAxes& a, F&& fn, Skip&& skip) {
  const uint32_t nxc = (nx + 255u) / 256u;
  const size_t ntasks = gradient_walk_tasks(nx, ny, nz);
  const uint32_t lane = threadIdx.x & 63u;
  // Workgroups are observed to be dealt round-robin over the 8 XCDs, each with an L2 of its own
  // (nothing promises it: this is for speed only, any placement computes the same).  The block
  // index is turned so that the workgroups of one XCD take consecutive tasks, and the rows of
  // y - 1 and y + 1 are then found in the L2 that a neighbour task has just filled.
  const uint32_t nb = gridDim.x;
  const uint32_t vb = (nb & 7u) ? blockIdx.x : (blockIdx.x & 7u) * (nb >> 3) + (blockIdx.x >> 3);
  for (size_t t = vb; t < ntasks; t += nb) {
    const uint32_t xc = (uint32_t)(t % nxc), y = (uint32_t)((t / nxc) % ny), zc = (uint32_t)(t / ((size_t)nxc * ny));
    const uint32_t x0 = xc * 256u + threadIdx.x;
    const uint32_t z0 = zc * kWalkZ, z1 = z0 + kWalkZ < nz ? z0 + kWalkZ : nz;
    if (skip(xc * 256u, x0, y, z0, z1)) continue;
    const bool in = x0 < nx;
    const uint32_t x = in ? x0 : nx - 1u;  // (lanes past the row read its last voxel)
    uint32_t xm, xp, ym, yp;
    float kx, ky;
    gradient_neighbours(x, nx, a.h1[0], a.h2[0], xm, xp, kx);
    gradient_neighbours(y, ny, a.h1[1], a.h2[1], ym, yp, ky);
    auto at = [&](uint32_t xx, uint32_t yy, uint32_t zz) { return (float)S[((size_t)zz * ny + yy) * nx + xx]; };
    float prev = at(x, y, z0 > 0u ? z0 - 1u : z0), cur = at(x, y, z0);
    for (uint32_t z = z0; z < z1; ++z) {
      uint32_t zm, zp;
      float kz;
      gradient_neighbours(z, nz, a.h1[2], a.h2[2], zm, zp, kz);
      const float next = zp != z ? at(x, y, zp) : cur;
      const float sym = ym != y ? at(x, ym, z) : cur, syp = yp != y ? at(x, yp, z) : cur;
      // every lane of the wave takes part in the two moves (the loop bounds are the workgroup's)
      const float left = __shfl_up(cur, 1), right = __shfl_down(cur, 1);
      const float sxm = xm == x ? cur : lane != 0u ? left : at(xm, y, z);
      const float sxp = xp == x ? cur : lane != 63u ? right : at(xp, y, z);
      fn(in, x, y, z, cur, gradient_magnitude(sxm, sxp, kx, sym, syp, ky, prev, next, kz));
      prev = cur;
      cur = next;
    }
  }
}
// The walk over every task
template <class T, class F>
__device__ __forceinline__ void gradient_walk(const T* __restrict__ S, uint32_t nx, uint32_t ny, uint32_t nz,
                                              const GradientAxes& a, F&& fn) {
  gradient_walk(S, nx, ny, nz, a, fn, [](uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) { return false; });
}

}  // namespace cvr
