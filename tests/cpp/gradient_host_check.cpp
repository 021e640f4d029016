// gradient_host_check.cpp - cvr_classify_gradient_host and its descriptor checks on the shapes
// where the neighbour indexing can go wrong (axes of 1, 2 and 3 voxels, every scalar type, a full
// 128 x 32 table), as a stand-alone host program: `make gradient-host-asan` builds it with
// cvr_medium.cpp's host code under -fsanitize=address,undefined and runs it.  Every array is
// allocated at its exact size, so a read or write past an end is an error the sanitizer reports.
// No GPU is touched.
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

cvr_gradient_transfer_desc desc_of(const std::vector<float>& table, uint32_t n, uint32_t m) {
  cvr_gradient_transfer_desc t{};
  t.n = n;
  t.m = m;
  t.table = table.data();
  t.lo = 10.0f, t.hi = 200.0f, t.glo = 0.0f, t.ghi = 90.0f;
  t.spacing[0] = 1.0f, t.spacing[1] = 2.0f, t.spacing[2] = 0.5f;
  return t;
}

template <class T>
void run_shape(uint32_t type, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t n, uint32_t m) {
  uint32_t seed = nx * 31u + ny * 17u + nz + type;
  const size_t count = (size_t)nx * ny * nz;
  std::vector<T> field(count);
  for (T& v : field) v = (T)(lcg(seed) >> 24);
  std::vector<float> table((size_t)n * m * 4);
  for (float& v : table) v = (float)(lcg(seed) >> 8) / 16777216.0f;
  const cvr_gradient_transfer_desc t = desc_of(table, n, m);
  const uint32_t res[3] = {nx, ny, nz};
  std::vector<float> d(count), a(4 * count), g(count);
  expect(cvr_classify_gradient_host(field.data(), type, res, &t, d.data(), a.data(), g.data()) == CVR_OK, "classify");
  expect(cvr_classify_gradient_host(field.data(), type, res, &t, nullptr, nullptr, nullptr) == CVR_OK, "no outputs");
  bool finite = true;
  for (size_t i = 0; i < count; ++i) finite = finite && std::isfinite(d[i]) && std::isfinite(g[i]) && a[4 * i + 3] == 1.0f;
  expect(finite, "finite outputs");
}

void run_all_types(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t n, uint32_t m) {
  run_shape<float>(CVR_SCALAR_F32, nx, ny, nz, n, m);
  run_shape<uint8_t>(CVR_SCALAR_U8, nx, ny, nz, n, m);
  run_shape<uint16_t>(CVR_SCALAR_U16, nx, ny, nz, n, m);
  run_shape<int16_t>(CVR_SCALAR_I16, nx, ny, nz, n, m);
}

void run_refusals() {
  std::vector<float> table(7 * 5 * 4, 0.5f);
  std::vector<uint8_t> field(60, 3);
  std::vector<float> d(60);
  const uint32_t res[3] = {5, 4, 3};
  auto call = [&](const cvr_gradient_transfer_desc& t) {
    return cvr_classify_gradient_host(field.data(), CVR_SCALAR_U8, res, &t, d.data(), nullptr, nullptr);
  };
  const cvr_gradient_transfer_desc good = desc_of(table, 7, 5);
  expect(call(good) == CVR_OK, "good descriptor");
  cvr_gradient_transfer_desc t = good;
  t.n = 1;
  expect(call(t) == CVR_ERR_INVALID, "n < 2");
  t = good, t.m = 1;
  expect(call(t) == CVR_ERR_INVALID, "m < 2");
  t = good, t.n = 65536, t.m = 65537;  // (the product does not fit 32 bits)
  expect(call(t) == CVR_ERR_INVALID, "n * m > 4096");
  t = good, t.flags = 1;
  expect(call(t) == CVR_ERR_INVALID, "flags");
  t = good, t.reserved = 1;
  expect(call(t) == CVR_ERR_INVALID, "reserved");
  t = good, t.table = nullptr;
  expect(call(t) == CVR_ERR_INVALID, "NULL table");
  t = good, t.hi = t.lo;
  expect(call(t) == CVR_ERR_INVALID, "hi <= lo");
  t = good, t.lo = NAN;
  expect(call(t) == CVR_ERR_INVALID, "lo NaN");
  t = good, t.glo = -1.0f;
  expect(call(t) == CVR_ERR_INVALID, "glo < 0");
  t = good, t.ghi = t.glo;
  expect(call(t) == CVR_ERR_INVALID, "ghi <= glo");
  t = good, t.ghi = INFINITY;
  expect(call(t) == CVR_ERR_INVALID, "ghi infinite");
  for (int k = 0; k < 3; ++k) {
    t = good, t.spacing[k] = 0.0f;
    expect(call(t) == CVR_ERR_INVALID, "spacing 0");
    t = good, t.spacing[k] = NAN;
    expect(call(t) == CVR_ERR_INVALID, "spacing NaN");
  }
  expect(cvr_classify_gradient_host(field.data(), 4, res, &good, d.data(), nullptr, nullptr) == CVR_ERR_INVALID,
         "scalar_type");
  expect(cvr_classify_gradient_host(nullptr, CVR_SCALAR_U8, res, &good, d.data(), nullptr, nullptr) == CVR_ERR_INVALID,
         "NULL field");
  expect(cvr_classify_gradient_host(field.data(), CVR_SCALAR_U8, nullptr, &good, d.data(), nullptr, nullptr) ==
             CVR_ERR_INVALID, "NULL res");
  expect(cvr_classify_gradient_host(field.data(), CVR_SCALAR_U8, res, nullptr, d.data(), nullptr, nullptr) ==
             CVR_ERR_INVALID, "NULL descriptor");
  const uint32_t none[3] = {5, 0, 3};
  expect(cvr_classify_gradient_host(nullptr, CVR_SCALAR_U8, none, &good, nullptr, nullptr, nullptr) == CVR_OK,
         "no voxels");
}

}  // namespace

int main() {
  // (x, y, z): the thin-axis shapes, then the full table's grid
  const uint32_t shapes[][3] = {{33, 9, 1}, {33, 1, 9}, {1, 33, 9}, {33, 9, 2}, {523, 5, 3}, {1, 1, 1}, {2, 2, 2}};
  for (const auto& s : shapes) run_all_types(s[0], s[1], s[2], 7, 5);
  run_all_types(16, 16, 16, 128, 32);
  run_all_types(33, 9, 2, 2, 2);
  run_all_types(5, 4, 3, 2048, 2);
  run_refusals();
  if (failures) return 1;
  printf("gradient_host_check: ok\n");
  return 0;
}
