// features_host_check.cpp - cvr_features_host and cvr_denoise_guided_host on the shapes where their
// indexing can go wrong (a ragged 24x17x19 grid, a 1x1x1 and a 2x1x3 grid, tiles ragged against
// every block size, an eye inside the box, rays that miss it, rays along its faces, NaN and
// infinite camera entries, every filter step against small and odd images), as a stand-alone host
// program: `make features-host-asan` builds it with the two host statements' code under
// -fsanitize=address,undefined and runs it.  Every array is allocated at its exact size, so a read
// or write past an end is an error the sanitizer reports.  No GPU is touched.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
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
float unit(uint32_t& s) { return (float)(lcg(s) >> 8) * (1.0f / 16777216.0f); }

struct Grid {
  std::vector<float> density, albedo;
  cvr_medium_desc m{};
};
void make_grid(Grid& g, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t seed) {
  const size_t n = (size_t)nx * ny * nz;
  g.density.resize(n);
  g.albedo.resize(4 * n);
  for (size_t i = 0; i < n; ++i) {
    const float u = unit(seed);
    g.density[i] = u < 0.4f ? 0.0f : u;
    for (int c = 0; c < 3; ++c) g.albedo[4 * i + c] = 0.2f + 0.8f * unit(seed);
    g.albedo[4 * i + 3] = 1.0f;
  }
  g.m.res[0] = nx, g.m.res[1] = ny, g.m.res[2] = nz;
  g.m.density = g.density.data();
  g.m.albedo = g.albedo.data();
  g.m.box_min[0] = -0.3f, g.m.box_min[1] = -0.2f, g.m.box_min[2] = -0.4f;
  g.m.box_max[0] = 0.5f, g.m.box_max[1] = 0.4f, g.m.box_max[2] = 0.8f;
  g.m.scale = 40.0f;
  g.m.max_density = 1.0f;
  g.m.roughness[0] = g.m.roughness[1] = 0.1f;
  g.m.eta = 1.04f;
}

struct Cam {
  float iv[12], r2v[2];
};
// right, up, forward as the columns, the eye in column 3
Cam camera(float ex, float ey, float ez, float fx, float fy, float fz, float fov) {
  Cam c{};
  const float l = std::sqrt(fx * fx + fy * fy + fz * fz);
  fx /= l, fy /= l, fz /= l;
  float rx = fz, ry = 0.0f, rz = -fx;  // forward x (0, 1, 0), up to sign
  const float rl = std::sqrt(rx * rx + rz * rz);
  if (rl > 0.0f) rx /= rl, rz /= rl;
  else rx = 1.0f;
  const float ux = fy * rz - fz * ry, uy = fz * rx - fx * rz, uz = fx * ry - fy * rx;
  const float M[12] = {rx, ux, fx, ex, ry, uy, fy, ey, rz, uz, fz, ez};
  for (int i = 0; i < 12; ++i) c.iv[i] = M[i];
  c.r2v[0] = c.r2v[1] = fov;
  return c;
}

void run_features(const Grid& g, const Cam& cam, uint32_t w, uint32_t h, uint32_t ox, uint32_t oy, int w2a,
                  const cvr_features_desc& d, bool expect_empty, const char* what) {
  const float full[2] = {64.0f, 48.0f};
  std::vector<float> rgba((size_t)w * h * 4, -1.0f), depth((size_t)w * h, -1.0f);
  const int r = cvr_features_host(&g.m, cam.iv, cam.r2v, full, w, h, ox, oy, w2a, &d, rgba.data(), depth.data());
  expect(r == CVR_OK, what);
  bool any = false, written = true;
  for (size_t i = 0; i < depth.size(); ++i) {
    any = any || rgba[4 * i + 3] != 0.0f;
    written = written && rgba[4 * i + 3] != -1.0f && depth[i] != -1.0f;
  }
  expect(written, "every pixel is written");
  if (expect_empty) expect(!any, what);
  expect(cvr_features_host(&g.m, cam.iv, cam.r2v, full, w, h, ox, oy, w2a, &d, rgba.data(), nullptr) == CVR_OK, what);
}

void run_guided(uint32_t w, uint32_t h, bool map, uint32_t passes, uint32_t seed) {
  const size_t px = (size_t)w * h;
  std::vector<float> s1(4 * px), s2(4 * px), f4(4 * px), fz(px), out(4 * px), var(px);
  for (size_t i = 0; i < 4 * px; ++i) {
    const float t = 1.5f * unit(seed);
    s1[i] = 8.0f * t;
    s2[i] = 8.0f * t * t;
    f4[i] = unit(seed);
  }
  for (size_t i = 0; i < px; ++i) fz[i] = unit(seed);
  s1[4 * (px / 2) + 1] = std::numeric_limits<float>::quiet_NaN();
  s2[4 * (px - 1)] = std::numeric_limits<float>::infinity();
  std::vector<uint32_t> counts((size_t)(w / 8) * (h / 8), 8u);
  if (map && !counts.empty()) counts.back() = 1u;
  const cvr_denoise_guided_desc d = {{passes, 4.0f, 0.01f, 0u}, 0.4f, 0.1f, 0.4f, 0u};
  const int r = cvr_denoise_guided_host(s1.data(), s2.data(), w, h, 8, map ? counts.data() : nullptr, &d, f4.data(),
                                        fz.data(), out.data(), (passes & 1u) ? var.data() : nullptr);
  expect(r == CVR_OK, "cvr_denoise_guided_host");
  for (size_t i = 0; i < 4 * px; ++i) expect(std::isfinite(out[i]), "a filtered value is finite");
}

}  // namespace

int main() {
  Grid ragged, one, thin;
  make_grid(ragged, 24, 17, 19, 5u);
  make_grid(one, 1, 1, 1, 6u);
  make_grid(thin, 2, 1, 3, 7u);
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const Cam oblique = camera(2.1f, 1.3f, -1.7f, -2.0f, -1.3f, 1.7f, 0.36f);
  const Cam inside = camera(0.1f, 0.1f, 0.2f, -0.4f, 0.7f, -0.85f, 1.0f);
  const Cam miss = camera(2.0f, 0.0f, 4.0f, 0.0f, 0.0f, -1.0f, 0.0f);       // a pencil beside the box
  const Cam in_face = camera(-3.0f, 0.4f, 0.1f, 1.0f, 0.0f, 0.0f, 0.0f);    // travels in the y = box_max plane
  const Cam on_edge = camera(0.5f, -0.2f, 4.0f, 0.0f, 0.0f, -1.0f, 0.0f);   // along an edge of the box
  const Cam wide = camera(0.1f, 0.1f, 0.2f, 0.0f, 0.0f, -1.0f, 1e30f);      // directions that overflow
  Cam broken = oblique;
  broken.iv[3] = nan;
  broken.iv[6] = inf;
  const cvr_features_desc descs[] = {{1.0f, 1.0f / 256.0f, 4096u, 0u}, {0.125f, 0.0f, 2048u, 0u}, {8.0f, 0.5f, 1u, 0u},
                                     {0.125f, 0.0f, 16u, 0u}};
  const uint32_t tiles[][4] = {{13, 7, 8, 8}, {40, 24, 8, 8}, {1, 1, 63, 47}, {64, 48, 0, 0}, {17, 9, 0, 39}};
  for (const Grid* g : {&ragged, &one, &thin})
    for (const auto& d : descs)
      for (const auto& t : tiles)
        for (int w2a = 0; w2a < 2; ++w2a) {
          run_features(*g, oblique, t[0], t[1], t[2], t[3], w2a, d, false, "oblique");
          run_features(*g, inside, t[0], t[1], t[2], t[3], w2a, d, false, "inside");
          run_features(*g, miss, t[0], t[1], t[2], t[3], w2a, d, true, "a miss is empty");
          run_features(*g, in_face, t[0], t[1], t[2], t[3], w2a, d, true, "a ray in a face plane is a miss");
          run_features(*g, on_edge, t[0], t[1], t[2], t[3], w2a, d, true, "a ray along an edge is a miss");
          if (t[0] * t[1] > 1024u) continue;  // (a NaN chord marches max_steps: the small tiles only)
          run_features(*g, wide, t[0], t[1], t[2], t[3], w2a, d, false, "overflowing directions");
          run_features(*g, broken, t[0], t[1], t[2], t[3], w2a, d, false, "NaN and inf in the camera");
        }
  // a medium outside the contract (NaN, inf and negative voxels) stays inside its arrays
  Grid bad;
  make_grid(bad, 5, 4, 3, 8u);
  bad.density[7] = nan, bad.density[11] = inf, bad.density[13] = -2.0f, bad.albedo[4 * 9] = nan;
  run_features(bad, inside, 40, 24, 8, 8, 0, descs[0], false, "a medium outside the contract");
  run_features(bad, oblique, 40, 24, 8, 8, 1, descs[1], false, "a medium outside the contract");

  const uint32_t shapes[][2] = {{13, 7}, {1, 1}, {3, 70}, {33, 9}};
  for (const auto& s : shapes)
    for (uint32_t passes = 1; passes <= 6; ++passes) run_guided(s[0], s[1], false, passes, s[0] * 7u + passes);
  for (uint32_t passes = 1; passes <= 6; ++passes) {
    run_guided(40, 24, true, passes, 90u + passes);
    run_guided(8, 8, true, passes, 70u + passes);
  }
  if (failures) {
    fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  printf("features_host_check: ok\n");
  return 0;
}
