// labels_host_check.cpp - cvr_classify_labels_host and the labelled descriptor's checks on the
// shapes where the indexing can go wrong (ragged voxel counts, one voxel, none; label bytes at and
// above m, 255 among them; m = 1 and the full 16 x 256 table; every scalar type; each output absent
// in turn), as a stand-alone host program: `make labels-host-asan` builds it with cvr_medium.cpp's
// host code under -fsanitize=address,undefined and runs it.  Every array is allocated at its exact
// size, so a read or write past an end is an error the sanitizer reports.  No GPU is touched.
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

size_t size_of(uint32_t type) { return type == CVR_SCALAR_U8 ? 1 : type == CVR_SCALAR_F32 ? 4 : 2; }

void run(uint32_t type, size_t n_voxels, uint32_t n, uint32_t m, uint32_t flags) {
  uint32_t seed = (uint32_t)n_voxels * 31u + n * 17u + m + type;
  std::vector<unsigned char> scalar(n_voxels * size_of(type));
  if (type == CVR_SCALAR_F32) {
    float* f = reinterpret_cast<float*>(scalar.data());
    for (size_t i = 0; i < n_voxels; ++i) f[i] = (float)(lcg(seed) >> 8) / 16777216.0f * 1.5f - 0.25f;
  } else {
    for (unsigned char& v : scalar) v = (unsigned char)(lcg(seed) >> 24);
  }
  std::vector<uint8_t> labels(n_voxels);
  for (size_t i = 0; i < n_voxels; ++i) labels[i] = (uint8_t)(lcg(seed) >> 24);  // every byte: at, above and below m
  if (n_voxels > 2) labels[0] = (uint8_t)(m < 256u ? m : 255u), labels[n_voxels - 1] = 255;
  std::vector<float> table((size_t)4 * n * m);
  for (float& v : table) v = (float)(lcg(seed) >> 8) / 16777216.0f;
  cvr_label_transfer_desc t{};
  t.n = n, t.m = m, t.flags = flags, t.table = table.data();
  t.lo = type == CVR_SCALAR_F32 ? 0.0f : type == CVR_SCALAR_I16 ? -30000.0f : 10.0f;
  t.hi = type == CVR_SCALAR_F32 ? 1.0f : type == CVR_SCALAR_U8 ? 240.0f : 30000.0f;
  std::vector<float> density(n_voxels), albedo(4 * n_voxels);
  std::vector<uint64_t> counts(256, 7u);
  const void* sp = n_voxels ? scalar.data() : nullptr;
  const uint8_t* lp = n_voxels ? labels.data() : nullptr;
  expect(cvr_classify_labels_host(sp, type, lp, n_voxels, &t, density.data(), albedo.data(), counts.data()) == CVR_OK,
         "all outputs");
  uint64_t sum = 0;
  std::vector<uint64_t> want(256, 0u);
  for (uint8_t l : labels) ++want[l];
  for (int b = 0; b < 256; ++b) sum += counts[b];
  expect(sum == n_voxels && counts == want, "counts are the labels' histogram");
  for (size_t i = 0; i < n_voxels; ++i) expect(albedo[4 * i + 3] == 1.0f, "albedo w is 1");
  // each output absent in turn, and all of them
  std::vector<float> d2(n_voxels), a2(4 * n_voxels);
  expect(cvr_classify_labels_host(sp, type, lp, n_voxels, &t, nullptr, a2.data(), nullptr) == CVR_OK, "no density");
  expect(cvr_classify_labels_host(sp, type, lp, n_voxels, &t, d2.data(), nullptr, counts.data()) == CVR_OK, "no albedo");
  expect(cvr_classify_labels_host(sp, type, lp, n_voxels, &t, nullptr, nullptr, nullptr) == CVR_OK, "no output");
  expect(n_voxels == 0 || (memcmp(d2.data(), density.data(), n_voxels * sizeof(float)) == 0 &&
                           memcmp(a2.data(), albedo.data(), 4 * n_voxels * sizeof(float)) == 0),
         "an absent output changes no other");
  if (m == 1u) {
    // one row: cvr_classify_host's bits, whatever the labels hold
    cvr_transfer_desc s{};
    s.n = n, s.flags = flags, s.table = table.data(), s.lo = t.lo, s.hi = t.hi;
    expect(cvr_classify_host(sp, type, n_voxels, &s, d2.data(), a2.data()) == CVR_OK, "cvr_classify_host");
    expect(n_voxels == 0 || (memcmp(d2.data(), density.data(), n_voxels * sizeof(float)) == 0 &&
                             memcmp(a2.data(), albedo.data(), 4 * n_voxels * sizeof(float)) == 0),
           "m = 1 is the scalar statement");
  }
}

void refusals() {
  const uint8_t s[4] = {1, 2, 3, 4}, l[4] = {0, 1, 2, 255};
  const float table[4 * 4] = {};
  auto code = [&](uint32_t n, uint32_t m, uint32_t flags, uint32_t reserved, const float* tab, float lo, float hi) {
    cvr_label_transfer_desc t{};
    t.n = n, t.m = m, t.flags = flags, t.reserved = reserved, t.table = tab, t.lo = lo, t.hi = hi;
    return cvr_classify_labels_host(s, CVR_SCALAR_U8, l, 4, &t, nullptr, nullptr, nullptr);
  };
  expect(code(2, 2, 0, 0, table, 0.0f, 1.0f) == CVR_OK, "a good descriptor");
  expect(code(1, 2, 0, 0, table, 0.0f, 1.0f) == CVR_ERR_INVALID, "n < 2");
  expect(code(2, 0, 0, 0, table, 0.0f, 1.0f) == CVR_ERR_INVALID, "m < 1");
  expect(code(2, 257, 0, 0, table, 0.0f, 1.0f) == CVR_ERR_INVALID, "m > 256");
  expect(code(4097, 1, 0, 0, table, 0.0f, 1.0f) == CVR_ERR_INVALID, "n * m > 4096");
  expect(code(2, 2, 4, 0, table, 0.0f, 1.0f) == CVR_ERR_INVALID, "unknown flags");
  expect(code(2, 2, 0, 1, table, 0.0f, 1.0f) == CVR_ERR_INVALID, "reserved");
  expect(code(2, 2, 0, 0, nullptr, 0.0f, 1.0f) == CVR_ERR_INVALID, "NULL table");
  expect(code(2, 2, 0, 0, table, 1.0f, 1.0f) == CVR_ERR_INVALID, "hi <= lo");
  cvr_label_transfer_desc t{};
  t.n = 2, t.m = 2, t.table = table, t.hi = 1.0f;
  expect(cvr_classify_labels_host(s, CVR_SCALAR_U8, nullptr, 4, &t, nullptr, nullptr, nullptr) == CVR_ERR_INVALID,
         "NULL labels");
  expect(cvr_classify_labels_host(s, 4u, l, 4, &t, nullptr, nullptr, nullptr) == CVR_ERR_INVALID, "scalar_type");
  expect(cvr_classify_labels_host(s, CVR_SCALAR_U8, l, 4, nullptr, nullptr, nullptr, nullptr) == CVR_ERR_INVALID,
         "NULL descriptor");
}

}  // namespace

int main() {
  const size_t sizes[] = {0, 1, 2, 15, 17, 37 * 29 * 23};
  const uint32_t types[] = {CVR_SCALAR_F32, CVR_SCALAR_U8, CVR_SCALAR_U16, CVR_SCALAR_I16};
  const uint32_t shapes[][2] = {{7, 1}, {2, 2}, {7, 5}, {16, 256}, {4096, 1}, {2, 256}};  // (n, m)
  for (size_t n_voxels : sizes)
    for (uint32_t type : types)
      for (const auto& nm : shapes)
        for (uint32_t flags = 0; flags < 4u; ++flags) run(type, n_voxels, nm[0], nm[1], flags);
  refusals();
  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  printf("labels_host_check: ok\n");
  return 0;
}
