// preview_host_check.cpp - cvr_preview_host on the shapes where its indexing can go wrong (a ragged
// 24x17x19 grid, a 1x1x1 and a 2x1x3 grid, whose gradient taps all clamp; tiles ragged against every
// block size; an eye inside the box, so that p - h leaves it; rays that miss the box or run along
// its faces; NaN and infinite camera entries; every kind of descriptor), as a stand-alone host
// program: `make preview-host-asan` builds it with the host statement's code under
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

void run(const Grid& g, const Cam& cam, uint32_t w, uint32_t h, uint32_t ox, uint32_t oy, int w2a,
         const cvr_preview_desc& d, bool expect_background, const char* what) {
  const float full[2] = {64.0f, 48.0f};
  std::vector<float> rgba((size_t)w * h * 4, -1.0f);
  expect(cvr_preview_host(&g.m, cam.iv, cam.r2v, full, w, h, ox, oy, w2a, &d, rgba.data()) == CVR_OK, what);
  bool written = true, background = true;
  for (size_t i = 0; i < (size_t)w * h; ++i) {
    written = written && rgba[4 * i + 3] != -1.0f;
    background = background && rgba[4 * i + 3] == 0.0f && rgba[4 * i] == d.background[0] &&
                 rgba[4 * i + 1] == d.background[1] && rgba[4 * i + 2] == d.background[2];
  }
  expect(written, "every pixel is written");
  if (expect_background) expect(background, what);
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
  const cvr_features_desc whole = {1.0f, 1.0f / 256.0f, 4096u, 0u}, fine = {0.125f, 0.0f, 2048u, 0u},
                          coarse = {8.0f, 0.5f, 1u, 0u}, capped = {0.125f, 0.0f, 16u, 0u};
  const cvr_preview_desc descs[] = {
      {whole, {0, 0, 0}, 0.3f, 0.7f, 0.2f, 4u, 0.05f, {0, 0, 0}, CVR_PREVIEW_HEADLIGHT},
      {fine, {0.3f, 1.0f, -0.4f}, 0.3f, 0.7f, 0.5f, 10u, 0.0f, {0.25f, 0.5f, 0.125f}, 0u},
      {coarse, {0, 0, 0}, 0.3f, 0.7f, 0.2f, 0u, 0.05f, {1.0f, 0.0f, 2.0f}, CVR_PREVIEW_UNSHADED},
      {capped, {-1e-18f, 0.0f, 0.0f}, 0.0f, 4.0f, 0.0f, 4u, 1e30f, {0, 0, 0}, 0u},
  };
  const uint32_t tiles[][4] = {{13, 7, 8, 8}, {40, 24, 8, 8}, {1, 1, 63, 47}, {64, 48, 0, 0}, {17, 9, 0, 39}};
  for (const Grid* g : {&ragged, &one, &thin})
    for (const auto& d : descs)
      for (const auto& t : tiles)
        for (int w2a = 0; w2a < 2; ++w2a) {
          run(*g, oblique, t[0], t[1], t[2], t[3], w2a, d, false, "oblique");
          run(*g, inside, t[0], t[1], t[2], t[3], w2a, d, false, "inside");
          run(*g, miss, t[0], t[1], t[2], t[3], w2a, d, true, "a miss is the background");
          run(*g, in_face, t[0], t[1], t[2], t[3], w2a, d, true, "a ray in a face plane is a miss");
          run(*g, on_edge, t[0], t[1], t[2], t[3], w2a, d, true, "a ray along an edge is a miss");
          if (t[0] * t[1] > 128u) continue;  // (a NaN chord marches max_steps, seven lookups each: the small tiles only)
          run(*g, wide, t[0], t[1], t[2], t[3], w2a, d, false, "overflowing directions");
          run(*g, broken, t[0], t[1], t[2], t[3], w2a, d, false, "NaN and inf in the camera");
        }
  // a medium outside the contract (NaN, inf and negative voxels) stays inside its arrays
  Grid bad;
  make_grid(bad, 5, 4, 3, 8u);
  bad.density[7] = nan, bad.density[11] = inf, bad.density[13] = -2.0f, bad.albedo[4 * 9] = nan;
  run(bad, inside, 40, 24, 8, 8, 0, descs[0], false, "a medium outside the contract");
  run(bad, oblique, 40, 24, 8, 8, 1, descs[1], false, "a medium outside the contract");

  // the refusals reach no array
  std::vector<float> px(4, 0.0f);
  const float full[2] = {64.0f, 48.0f};
  cvr_preview_desc r = descs[0];
  expect(cvr_preview_host(&ragged.m, oblique.iv, oblique.r2v, full, 1, 1, 0, 0, 0, nullptr, px.data()) == CVR_ERR_INVALID,
         "a NULL descriptor");
  r.march.step = 9.0f;
  expect(cvr_preview_host(&ragged.m, oblique.iv, oblique.r2v, full, 1, 1, 0, 0, 0, &r, px.data()) == CVR_ERR_INVALID, "step");
  r = descs[0], r.flags = 4u;
  expect(cvr_preview_host(&ragged.m, oblique.iv, oblique.r2v, full, 1, 1, 0, 0, 0, &r, px.data()) == CVR_ERR_INVALID, "flags");
  r = descs[0], r.shininess_log2 = 11u;
  expect(cvr_preview_host(&ragged.m, oblique.iv, oblique.r2v, full, 1, 1, 0, 0, 0, &r, px.data()) == CVR_ERR_INVALID,
         "shininess_log2");
  r = descs[1], r.light[0] = r.light[1] = r.light[2] = 0.0f;
  expect(cvr_preview_host(&ragged.m, oblique.iv, oblique.r2v, full, 1, 1, 0, 0, 0, &r, px.data()) == CVR_ERR_INVALID,
         "a zero light");
  if (failures) {
    fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  printf("preview_host_check: ok\n");
  return 0;
}
