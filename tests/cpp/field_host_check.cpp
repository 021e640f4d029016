// field_host_check.cpp - cvr_field_stats_host and cvr_field_histogram_host on the shapes where the
// neighbour indexing can go wrong (axes of 1, 2 and 3 voxels, every scalar type), on a field of
// NaNs, infinities and signed zeros, and at the smallest and the largest bin counts, as a
// stand-alone host program: `make field-host-asan` builds it with cvr_field_api.cpp's host code
// under -fsanitize=address,undefined and runs it.  Every array is allocated at its exact size, so a
// read or write past an end is an error the sanitizer reports.  No GPU is touched.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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

cvr_field_desc field_of(const void* scalar, uint32_t type, uint32_t nx, uint32_t ny, uint32_t nz) {
  cvr_field_desc f{};
  f.res[0] = nx, f.res[1] = ny, f.res[2] = nz;
  f.scalar_type = type;
  f.scalar = scalar;
  f.spacing[0] = 1.0f, f.spacing[1] = 2.0f, f.spacing[2] = 0.5f;
  return f;
}

cvr_histogram_desc bins_of(uint32_t n, uint32_t m) {
  cvr_histogram_desc h{};
  h.n = n, h.m = m;
  h.lo = 10.0f, h.hi = 200.0f, h.glo = 0.0f, h.ghi = 90.0f;
  return h;
}

// Both calls on one field; the counts' sum is the voxel count
void run_field(const cvr_field_desc& f, uint32_t n, uint32_t m) {
  const size_t voxels = (size_t)f.res[0] * f.res[1] * f.res[2];
  struct cvr_field_stats st;
  expect(cvr_field_stats_host(&f, &st) == CVR_OK, "stats");
  expect(st.nan_values <= voxels && st.nan_gradients <= voxels && st.reserved == 0u, "stats counts");
  const cvr_histogram_desc h = bins_of(n, m);
  std::vector<uint32_t> counts((size_t)n * m, 0xDEADBEEFu);  // the call clears them itself
  expect(cvr_field_histogram_host(&f, &h, counts.data()) == CVR_OK, "histogram");
  uint64_t sum = 0;
  for (uint32_t c : counts) sum += c;
  expect(sum == voxels, "counts sum to the voxel count");
}

template <class T>
void run_shape(uint32_t type, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t n, uint32_t m) {
  uint32_t seed = nx * 31u + ny * 17u + nz + type;
  std::vector<T> field((size_t)nx * ny * nz);
  for (T& v : field) v = (T)(lcg(seed) >> 24);
  run_field(field_of(field.data(), type, nx, ny, nz), n, m);
}

void run_all_types(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t n, uint32_t m) {
  run_shape<float>(CVR_SCALAR_F32, nx, ny, nz, n, m);
  run_shape<uint8_t>(CVR_SCALAR_U8, nx, ny, nz, n, m);
  run_shape<uint16_t>(CVR_SCALAR_U16, nx, ny, nz, n, m);
  run_shape<int16_t>(CVR_SCALAR_I16, nx, ny, nz, n, m);
}

void run_nonfinite() {
  const uint32_t nx = 10, ny = 9, nz = 11;
  uint32_t seed = 71;
  std::vector<float> field((size_t)nx * ny * nz);
  for (float& v : field) v = (float)(lcg(seed) >> 8) / 65536.0f;
  auto at = [&](uint32_t x, uint32_t y, uint32_t z) -> float& { return field[((size_t)z * ny + y) * nx + x]; };
  at(2, 2, 2) = NAN, at(0, 0, 0) = NAN;
  at(4, 5, 5) = INFINITY, at(6, 5, 5) = INFINITY;  // (5, 5, 5): inf - inf
  at(9, 8, 10) = -INFINITY;
  at(3, 3, 3) = -0.0f, at(4, 3, 3) = 0.0f;
  const cvr_field_desc f = field_of(field.data(), CVR_SCALAR_F32, nx, ny, nz);
  run_field(f, 7, 5);
  run_field(f, 256, 256);
  run_field(f, 65536, 1);
  struct cvr_field_stats st;
  expect(cvr_field_stats_host(&f, &st) == CVR_OK, "nonfinite stats");
  expect(st.nan_values == 2 && st.nan_gradients > 2 && st.vmin == -INFINITY && st.vmax == INFINITY &&
             st.gmax == INFINITY, "nonfinite statistics");
  std::vector<float> nans(24, NAN);
  const cvr_field_desc g = field_of(nans.data(), CVR_SCALAR_F32, 4, 3, 2);
  expect(cvr_field_stats_host(&g, &st) == CVR_OK && st.vmin == INFINITY && st.vmax == -INFINITY && st.gmax == 0.0f &&
             st.nan_values == 24 && st.nan_gradients == 24, "a field of NaNs");
  run_field(g, 2, 2);
}

void run_refusals() {
  std::vector<uint16_t> field(60, 3);
  std::vector<uint32_t> counts(35);
  const cvr_field_desc good = field_of(field.data(), CVR_SCALAR_U16, 5, 4, 3);
  const cvr_histogram_desc bins = bins_of(7, 5);
  struct cvr_field_stats st;
  auto hist = [&](const cvr_field_desc& f, const cvr_histogram_desc& h) {
    return cvr_field_histogram_host(&f, &h, counts.data());
  };
  expect(hist(good, bins) == CVR_OK, "good descriptors");
  expect(cvr_field_stats_host(nullptr, &st) == CVR_ERR_INVALID, "NULL field");
  expect(cvr_field_stats_host(&good, nullptr) == CVR_ERR_INVALID, "NULL stats");
  expect(cvr_field_histogram_host(&good, nullptr, counts.data()) == CVR_ERR_INVALID, "NULL histogram");
  expect(cvr_field_histogram_host(&good, &bins, nullptr) == CVR_ERR_INVALID, "NULL counts");
  cvr_field_desc f = good;
  f.res[1] = 0, f.scalar = nullptr;
  expect(hist(f, bins) == CVR_ERR_INVALID && cvr_field_stats_host(&f, &st) == CVR_ERR_INVALID, "zero extent");
  f = good, f.res[0] = 65536u, f.res[1] = 65536u, f.res[2] = 1u, f.scalar = nullptr;
  expect(hist(f, bins) == CVR_ERR_INVALID && cvr_field_stats_host(&f, &st) == CVR_ERR_INVALID, "2^32 voxels");
  f = good, f.res[0] = f.res[1] = f.res[2] = 0xFFFFFFFFu, f.scalar = nullptr;  // (the product does not fit 64 bits)
  expect(hist(f, bins) == CVR_ERR_INVALID, "2^96 voxels");
  f = good, f.scalar_type = 4;
  expect(hist(f, bins) == CVR_ERR_INVALID, "scalar_type");
  f = good, f.reserved = 1;
  expect(hist(f, bins) == CVR_ERR_INVALID, "reserved");
  f = good, f.scalar = nullptr;
  expect(hist(f, bins) == CVR_ERR_INVALID, "NULL scalar");
  f = good, f.scalar = reinterpret_cast<const uint8_t*>(field.data()) + 1;
  expect(hist(f, bins) == CVR_ERR_INVALID, "misaligned scalar");
  for (int k = 0; k < 3; ++k) {
    f = good, f.spacing[k] = 0.0f;
    expect(hist(f, bins) == CVR_ERR_INVALID && cvr_field_stats_host(&f, &st) == CVR_ERR_INVALID, "spacing 0");
    f = good, f.spacing[k] = NAN;
    expect(hist(f, bins) == CVR_ERR_INVALID, "spacing NaN");
    // m == 1: the spacing is not judged
    expect(hist(f, bins_of(35, 1)) == CVR_OK, "m = 1 ignores the spacing");
  }
  cvr_histogram_desc h = bins;
  h.n = 1;
  expect(hist(good, h) == CVR_ERR_INVALID, "n < 2");
  h = bins, h.m = 0;
  expect(hist(good, h) == CVR_ERR_INVALID, "m < 1");
  h = bins, h.n = 65536, h.m = 65537;  // (the product does not fit 32 bits)
  expect(hist(good, h) == CVR_ERR_INVALID, "n * m > 65536");
  h = bins, h.flags = 1;
  expect(hist(good, h) == CVR_ERR_INVALID, "flags");
  h = bins, h.reserved = 1;
  expect(hist(good, h) == CVR_ERR_INVALID, "histogram reserved");
  h = bins, h.hi = h.lo;
  expect(hist(good, h) == CVR_ERR_INVALID, "hi <= lo");
  h = bins, h.lo = NAN;
  expect(hist(good, h) == CVR_ERR_INVALID, "lo NaN");
  h = bins, h.glo = -1.0f;
  expect(hist(good, h) == CVR_ERR_INVALID, "glo < 0");
  h = bins, h.ghi = INFINITY;
  expect(hist(good, h) == CVR_ERR_INVALID, "ghi infinite");
  h = bins_of(35, 1), h.glo = NAN, h.ghi = -1.0f;
  expect(hist(good, h) == CVR_OK, "m = 1 ignores glo and ghi");
  uint32_t geo[8];
  expect(cvr_debug_field_geometry(geo) == CVR_OK && geo[7] == 5u && cvr_debug_field_geometry(nullptr) == CVR_ERR_INVALID,
         "geometry");
}

}  // namespace

int main() {
  // (x, y, z): the thin-axis shapes
  const uint32_t shapes[][3] = {{33, 9, 1}, {33, 1, 9}, {1, 33, 9}, {33, 9, 2}, {523, 5, 3}, {1, 1, 1}, {2, 2, 2}};
  for (const auto& s : shapes) {
    run_all_types(s[0], s[1], s[2], 7, 5);
    run_all_types(s[0], s[1], s[2], 256, 1);
  }
  run_all_types(16, 16, 16, 256, 256);
  run_all_types(33, 9, 2, 2, 2);
  run_all_types(5, 4, 3, 2, 1);
  run_nonfinite();
  run_refusals();
  if (failures) return 1;
  printf("field_host_check: ok\n");
  return 0;
}
