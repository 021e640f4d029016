// clip_host_check.cpp - cvr_clip_host and the clip descriptor's checks on the shapes where the
// indexing can go wrong (a ragged 37x29x21 grid, axes of one voxel, crops off the leaf grid and
// past the grid, an empty crop, one to eight planes, each output absent in turn), as a stand-alone
// host program: `make clip-host-asan` builds it with cvr_medium.cpp's host code under
// -fsanitize=address,undefined and runs it.  Every array is allocated at its exact size, so a read
// or write past an end is an error the sanitizer reports.  No GPU is touched.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvr.h"

namespace {

int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) {
    fprintf(stderr, "FAIL: %s\n", what);
    ++failures;
  }
}

uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

cvr_clip_desc region(const uint32_t lo[3], const uint32_t hi[3], uint32_t n_planes) {
  static const float planes[CVR_CLIP_MAX_PLANES][4] = {
      {0.6f, -0.35f, 0.72f, -9.3f}, {-1.0f, -1.0f, -0.25f, 45.5f}, {1.0f, -1.0f, 0.0f, 0.0f}, {0.0f, -1.0f, 0.0f, 26.25f},
      {0.0f, 0.0f, 1.0f, -1.0f},    {0.0f, 0.0f, -1.0f, 18.0f},    {0.37f, 0.41f, 0.83f, -11.0f}, {0.0f, 1.0f, 0.0f, -0.0f}};
  cvr_clip_desc d{};
  memcpy(d.lo, lo, sizeof(d.lo));
  memcpy(d.hi, hi, sizeof(d.hi));
  d.n_planes = n_planes;
  memcpy(d.planes, planes, sizeof(planes));
  return d;
}

// the statement, restated: the kept mask the call must return
bool keeps(const cvr_clip_desc& d, const uint32_t res[3], uint32_t x, uint32_t y, uint32_t z) {
  const uint32_t c[3] = {x, y, z};
  for (int a = 0; a < 3; ++a)
    if (c[a] < d.lo[a] || c[a] >= (d.hi[a] < res[a] ? d.hi[a] : res[a])) return false;
  for (uint32_t k = 0; k < d.n_planes; ++k) {
    volatile float ax = d.planes[k][0] * (float)x, by = d.planes[k][1] * (float)y, cz = d.planes[k][2] * (float)z;
    volatile float s = ax + by;
    s = s + cz;
    s = s + d.planes[k][3];
    if (!(s >= 0.0f)) return false;
  }
  return true;
}

void run(uint32_t nx, uint32_t ny, uint32_t nz, const cvr_clip_desc& d) {
  const uint32_t res[3] = {nx, ny, nz};
  const size_t n = (size_t)nx * ny * nz;
  uint32_t seed = nx * 31u + ny * 17u + nz + d.n_planes;
  std::vector<float> dens(n), alb(4 * n);
  for (float& v : dens) v = (float)(lcg(seed) >> 8) / 16777216.0f + 0.5f;
  for (float& v : alb) v = (float)(lcg(seed) >> 8) / 16777216.0f;
  const std::vector<float> dens0 = dens, alb0 = alb;
  std::vector<uint8_t> keep(n, 7);
  expect(cvr_clip_host(res, &d, dens.data(), alb.data(), keep.data()) == CVR_OK, "all three arrays");
  bool ok = true;
  size_t i = 0;
  for (uint32_t z = 0; z < nz; ++z)
    for (uint32_t y = 0; y < ny; ++y)
      for (uint32_t x = 0; x < nx; ++x, ++i) {
        const bool k = keeps(d, res, x, y, z);
        ok = ok && keep[i] == (k ? 1 : 0);
        ok = ok && (k ? dens[i] == dens0[i] : (dens[i] == 0.0f && !std::signbit(dens[i])));
        ok = ok && memcmp(&alb[4 * i], k ? &alb0[4 * i] : &alb0[0], 16) == 0;
      }
  expect(ok, "the statement's values");
  // each output absent in turn, and all of them
  std::vector<float> d2 = dens0, a2 = alb0;
  std::vector<uint8_t> k2(n);
  expect(cvr_clip_host(res, &d, d2.data(), nullptr, nullptr) == CVR_OK && d2 == dens, "density alone");
  expect(cvr_clip_host(res, &d, nullptr, a2.data(), nullptr) == CVR_OK && a2 == alb, "albedo alone");
  expect(cvr_clip_host(res, &d, nullptr, nullptr, k2.data()) == CVR_OK && k2 == keep, "keep alone");
  expect(cvr_clip_host(res, &d, nullptr, nullptr, nullptr) == CVR_OK, "no outputs");
}

void run_refusals() {
  const uint32_t res[3] = {5, 4, 3}, lo[3] = {0, 0, 0}, hi[3] = {5, 4, 3};
  std::vector<uint8_t> keep(60);
  auto call = [&](const cvr_clip_desc* d) { return cvr_clip_host(res, d, nullptr, nullptr, keep.data()); };
  const cvr_clip_desc good = region(lo, hi, 8);
  expect(call(&good) == CVR_OK, "good descriptor");
  expect(call(nullptr) == CVR_ERR_INVALID, "NULL descriptor");
  cvr_clip_desc d = good;
  d.flags = 1;
  expect(call(&d) == CVR_ERR_INVALID, "flags");
  d = good, d.n_planes = 9;
  expect(call(&d) == CVR_ERR_INVALID, "n_planes > 8");
  d = good, d.n_planes = 0xFFFFFFFFu;
  expect(call(&d) == CVR_ERR_INVALID, "n_planes huge");
  d = good, d.lo[2] = 3, d.hi[2] = 2;
  expect(call(&d) == CVR_ERR_INVALID, "lo > hi");
  d = good, d.planes[7][0] = NAN;
  expect(call(&d) == CVR_ERR_INVALID, "NaN coefficient");
  d = good, d.planes[0][3] = INFINITY;
  expect(call(&d) == CVR_ERR_INVALID, "infinite coefficient");
  d = good, d.planes[3][1] = 0.0f;
  expect(call(&d) == CVR_ERR_INVALID, "zero normal");
  d = good, d.n_planes = 3, d.planes[3][1] = 0.0f, d.planes[4][0] = NAN;
  expect(call(&d) == CVR_OK, "entries from n_planes on are ignored");
  const uint32_t none[3] = {5, 0, 3};
  expect(cvr_clip_host(none, &good, nullptr, nullptr, nullptr) == CVR_ERR_INVALID, "empty grid");
  expect(cvr_clip_host(nullptr, &good, nullptr, nullptr, nullptr) == CVR_ERR_INVALID, "NULL res");
  const uint32_t huge[3] = {65536, 65536, 2};
  expect(cvr_clip_host(huge, &good, nullptr, nullptr, nullptr) == CVR_ERR_INVALID, "more than 2^32 - 1 voxels");
  expect(sizeof(cvr_clip_desc) == 160, "sizeof(cvr_clip_desc)");
}

}  // namespace

int main() {
  const uint32_t zero[3] = {0, 0, 0}, all[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
  const uint32_t lo[3] = {3, 9, 2}, hi[3] = {30, 17, 40}, at[3] = {5, 5, 5}, past[3] = {40, 40, 40};
  // (x, y, z): the ragged grid, axes of one voxel, one voxel
  const uint32_t shapes[][3] = {{37, 29, 21}, {37, 29, 1}, {37, 1, 21}, {1, 29, 21}, {1, 1, 1}, {9, 8, 7}};
  for (const auto& s : shapes) {
    for (uint32_t n_planes : {0u, 1u, 2u, 8u}) {
      run(s[0], s[1], s[2], region(zero, all, n_planes));
      run(s[0], s[1], s[2], region(lo, hi, n_planes));
    }
    run(s[0], s[1], s[2], region(at, at, 0));      // an empty crop
    run(s[0], s[1], s[2], region(past, all, 0));   // a crop that starts past the grid
  }
  run_refusals();
  if (failures) return 1;
  printf("clip_host_check: ok\n");
  return 0;
}
