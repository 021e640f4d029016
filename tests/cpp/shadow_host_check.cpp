// shadow_host_check.cpp - cvr_light_volume_host and cvr_preview_shadowed_host on the shapes where
// their indexing can go wrong (a ragged 24x17x19 medium, a 1x1x1 and a 2x1x3 one; light grids of one
// node, of one node on two axes, ragged, and finer than the medium, whose lookup taps clamp on every
// side; axis-aligned lights, whose chord has infinite slabs; an eye inside the box; rays that miss;
// NaN and infinite camera entries; a volume outside [0, 1]), as a stand-alone host program:
// `make shadow-host-asan` builds it with the host statements' code under
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

// the volume of `v` for `g`, every node written and inside [0, 1]
std::vector<float> build(const Grid& g, const cvr_light_volume_desc& v, int w2a, bool in_contract, const char* what) {
  std::vector<float> S((size_t)v.res[0] * v.res[1] * v.res[2], -1.0f);
  expect(cvr_light_volume_host(&g.m, w2a, &v, S.data()) == CVR_OK, what);
  bool ok = true;
  for (float s : S) ok = ok && (in_contract ? s >= 0.0f && s <= 1.0f : s != -1.0f);
  expect(ok, "every node is written, inside [0, 1]");
  return S;
}

void run(const Grid& g, const Cam& cam, uint32_t w, uint32_t h, uint32_t ox, uint32_t oy, int w2a, const cvr_preview_desc& d,
         const cvr_light_volume_desc& v, const std::vector<float>& S, float shadow, bool expect_background, const char* what) {
  const float full[2] = {64.0f, 48.0f};
  std::vector<float> rgba((size_t)w * h * 4, -1.0f);
  expect(cvr_preview_shadowed_host(&g.m, cam.iv, cam.r2v, full, w, h, ox, oy, w2a, &d, &v, S.data(), shadow, rgba.data()) == CVR_OK,
         what);
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
  const Cam miss = camera(2.0f, 0.0f, 4.0f, 0.0f, 0.0f, -1.0f, 0.0f);  // a pencil beside the box
  const Cam wide = camera(0.1f, 0.1f, 0.2f, 0.0f, 0.0f, -1.0f, 1e30f);  // directions that overflow
  Cam broken = oblique;
  broken.iv[3] = nan;
  broken.iv[6] = inf;
  const cvr_features_desc whole = {1.0f, 1.0f / 256.0f, 4096u, 0u}, fine = {0.125f, 0.0f, 2048u, 0u},
                          coarse = {8.0f, 0.5f, 1u, 0u};
  const cvr_preview_desc descs[] = {
      {whole, {0, 0, 0}, 0.3f, 0.7f, 0.2f, 4u, 0.05f, {0, 0, 0}, 0u},
      {fine, {nan, inf, 0}, 0.3f, 0.7f, 0.5f, 10u, 0.0f, {0.25f, 0.5f, 0.125f}, 0u},  // (the light is not read)
      {coarse, {0, 0, 0}, 0.3f, 0.7f, 0.2f, 0u, 0.05f, {1.0f, 0.0f, 2.0f}, CVR_PREVIEW_UNSHADED},
  };
  const cvr_light_volume_desc volumes[] = {
      {{1, 1, 1}, 0u, {0.3f, 1.0f, -0.4f}, 0.0f, whole},    {{13, 11, 9}, 0u, {0.0f, 0.0f, 1.0f}, 0.0f, whole},
      {{1, 7, 1}, 0u, {-1.0f, 0.0f, 0.0f}, 0.0f, fine},     {{40, 3, 33}, 0u, {0.0f, -1e-18f, 0.0f}, 0.0f, coarse},
      {{5, 4, 70}, 0u, {1e18f, 1e18f, -1e18f}, 0.0f, whole},
  };
  const uint32_t tiles[][4] = {{13, 7, 8, 8}, {40, 24, 8, 8}, {1, 1, 63, 47}, {17, 9, 0, 39}};
  for (const Grid* g : {&ragged, &one, &thin})
    for (const auto& v : volumes)
      for (int w2a = 0; w2a < 2; ++w2a) {
        const std::vector<float> S = build(*g, v, w2a, true, "the light volume");
        for (const auto& d : descs)
          for (const auto& t : tiles) {
            const float shadow = (&d == &descs[0]) ? 0.5f : 1.0f;
            run(*g, oblique, t[0], t[1], t[2], t[3], w2a, d, v, S, shadow, false, "oblique");
            run(*g, inside, t[0], t[1], t[2], t[3], w2a, d, v, S, shadow, false, "inside");
            run(*g, miss, t[0], t[1], t[2], t[3], w2a, d, v, S, shadow, true, "a miss is the background");
            if (t[0] * t[1] > 128u) continue;  // (a NaN chord marches max_steps: the small tiles only)
            run(*g, wide, t[0], t[1], t[2], t[3], w2a, d, v, S, shadow, false, "overflowing directions");
            run(*g, broken, t[0], t[1], t[2], t[3], w2a, d, v, S, shadow, false, "NaN and inf in the camera");
          }
      }
  // a medium and a volume outside the contract (NaN, inf and negative values) stay inside their arrays
  Grid bad;
  make_grid(bad, 5, 4, 3, 8u);
  bad.density[7] = nan, bad.density[11] = inf, bad.density[13] = -2.0f, bad.albedo[4 * 9] = nan;
  std::vector<float> S = build(bad, volumes[1], 0, false, "a medium outside the contract");
  S[3] = nan, S[5] = -inf, S[7] = 1e30f;
  run(bad, inside, 40, 24, 8, 8, 0, descs[0], volumes[1], S, 1.0f, false, "a medium outside the contract");
  run(bad, oblique, 40, 24, 8, 8, 0, descs[1], volumes[1], S, 0.0f, false, "a medium outside the contract");

  // the refusals reach no array
  std::vector<float> px(4, 0.0f), node(1, 0.0f);
  const float full[2] = {64.0f, 48.0f};
  cvr_light_volume_desc v = volumes[0];
  expect(cvr_light_volume_host(&ragged.m, 0, nullptr, node.data()) == CVR_ERR_INVALID, "a NULL volume descriptor");
  v.flags = 1u;
  expect(cvr_light_volume_host(&ragged.m, 0, &v, node.data()) == CVR_ERR_INVALID, "volume flags");
  v = volumes[0], v.res[1] = 1025u;
  expect(cvr_light_volume_host(&ragged.m, 0, &v, node.data()) == CVR_ERR_INVALID, "res above 1024");
  v = volumes[0], v.res[0] = v.res[1] = 1024u, v.res[2] = 129u;
  expect(cvr_light_volume_host(&ragged.m, 0, &v, node.data()) == CVR_ERR_INVALID, "more than 2^27 nodes");
  v = volumes[0], v.light[0] = v.light[1] = v.light[2] = 0.0f;
  expect(cvr_light_volume_host(&ragged.m, 0, &v, node.data()) == CVR_ERR_INVALID, "a zero light");
  v = volumes[0], v.march.step = 9.0f;
  expect(cvr_light_volume_host(&ragged.m, 0, &v, node.data()) == CVR_ERR_INVALID, "the volume's step");
  cvr_preview_desc r = descs[0];
  auto shadowed = [&](const cvr_preview_desc* d, const cvr_light_volume_desc* vd, float shadow) {
    return cvr_preview_shadowed_host(&ragged.m, oblique.iv, oblique.r2v, full, 1, 1, 0, 0, 0, d, vd, node.data(), shadow, px.data());
  };
  expect(shadowed(&r, &volumes[0], 0.5f) == CVR_OK, "one pixel, one node");
  expect(shadowed(nullptr, &volumes[0], 0.5f) == CVR_ERR_INVALID, "a NULL descriptor");
  r.march.step = 9.0f;
  expect(shadowed(&r, &volumes[0], 0.5f) == CVR_ERR_INVALID, "step");
  r = descs[0], r.flags = CVR_PREVIEW_HEADLIGHT;
  expect(shadowed(&r, &volumes[0], 0.5f) == CVR_ERR_INVALID, "the headlight");
  r = descs[0];
  expect(shadowed(&r, &volumes[0], 1.5f) == CVR_ERR_INVALID && shadowed(&r, &volumes[0], nan) == CVR_ERR_INVALID, "the strength");
  expect(shadowed(&r, nullptr, 0.5f) == CVR_ERR_INVALID && shadowed(&r, &v, 0.5f) == CVR_ERR_INVALID, "the volume's descriptor");
  if (failures) {
    fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  printf("shadow_host_check: ok\n");
  return 0;
}
