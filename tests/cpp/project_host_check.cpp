// project_host_check.cpp - cvr_field_project_host on the shapes where its indexing can go wrong (a
// ragged 37x29x23 field of every scalar type, a 5x1x3 field with an axis of one voxel, a 2x2x2 and a
// 1x1x1 field, whose gradient taps all clamp; an f32 field with NaN and infinite voxels and one that
// is all NaN; tiles ragged against every block size; an eye inside the box, so that p - h leaves
// it; rays that miss the box; NaN and infinite camera entries; every mode), as a stand-alone host
// program: `make project-host-asan` builds it with the host statement's code under
// -fsanitize=address,undefined and runs it.  Every array is allocated at its exact size, so a read
// or write past an end is an error the sanitizer reports.  No GPU is touched.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

// A field of `type` at its exact size in bytes
struct Field {
  std::vector<uint8_t> bytes;
  cvr_field_desc f{};
};
void make_field(Field& g, uint32_t type, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t seed) {
  const size_t n = (size_t)nx * ny * nz, size = type == CVR_SCALAR_U8 ? 1 : type == CVR_SCALAR_F32 ? 4 : 2;
  g.bytes.resize(n * size);
  for (size_t i = 0; i < n; ++i) {
    const uint32_t r = lcg(seed) >> 8;
    if (type == CVR_SCALAR_F32) {
      const float v = (float)r * (1.0f / 16777216.0f);
      memcpy(&g.bytes[4 * i], &v, 4);
    } else if (type == CVR_SCALAR_U8) {
      g.bytes[i] = (uint8_t)r;
    } else {
      const uint16_t v = (uint16_t)r;  // (i16: the same bits, both signs)
      memcpy(&g.bytes[2 * i], &v, 2);
    }
  }
  g.f.res[0] = nx, g.f.res[1] = ny, g.f.res[2] = nz;
  g.f.scalar_type = type;
  g.f.scalar = g.bytes.data();
}
void set_f32(Field& g, size_t i, float v) { memcpy(&g.bytes[4 * i], &v, 4); }

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

cvr_project_desc desc(uint32_t mode, float lo, float hi, float iso) {
  cvr_project_desc d{};
  d.mode = mode;
  d.flags = CVR_PROJECT_HEADLIGHT;
  d.box_min[0] = -0.3f, d.box_min[1] = -0.2f, d.box_min[2] = -0.4f;
  d.box_max[0] = 0.5f, d.box_max[1] = 0.4f, d.box_max[2] = 0.8f;
  d.step = 1.0f, d.max_steps = 4096u;
  d.lo = lo, d.hi = hi, d.iso = iso, d.refine = 4u;
  d.ambient = 0.3f, d.diffuse = 0.7f, d.specular = 0.2f, d.shininess_log2 = 4u;
  d.colour[0] = d.colour[1] = d.colour[2] = 1.0f;
  d.background[0] = 0.25f, d.background[1] = 0.5f, d.background[2] = 0.125f;
  return d;
}

const float kFull[2] = {64.0f, 48.0f};

void run(const Field& g, const Cam& cam, uint32_t w, uint32_t h, uint32_t ox, uint32_t oy, const cvr_project_desc& d,
         bool planes, bool expect_background, const char* what) {
  std::vector<float> rgba((size_t)w * h * 4, -1.0f), value((size_t)w * h, -1.0f), depth((size_t)w * h, -1.0f);
  expect(cvr_field_project_host(&g.f, &d, cam.iv, cam.r2v, kFull, w, h, ox, oy, rgba.data(), planes ? value.data() : nullptr,
                                planes ? depth.data() : nullptr) == CVR_OK, what);
  bool written = true, background = true;
  for (size_t i = 0; i < (size_t)w * h; ++i) {
    written = written && rgba[4 * i + 3] != -1.0f && (!planes || depth[i] != -1.0f);
    background = background && rgba[4 * i + 3] == 0.0f && rgba[4 * i] == d.background[0] &&
                 rgba[4 * i + 1] == d.background[1] && rgba[4 * i + 2] == d.background[2] &&
                 (!planes || (value[i] == 0.0f && depth[i] == 0.0f));
  }
  expect(written, "every pixel is written");
  if (expect_background) expect(background, what);
}

}  // namespace

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  Field ragged[4], thin, cube, one, bad, all_nan;
  for (uint32_t t = 0; t < 4; ++t) make_field(ragged[t], t, 37, 29, 23, 5u + t);
  make_field(thin, CVR_SCALAR_U16, 5, 1, 3, 11u);
  make_field(cube, CVR_SCALAR_I16, 2, 2, 2, 12u);
  make_field(one, CVR_SCALAR_U8, 1, 1, 1, 13u);
  make_field(bad, CVR_SCALAR_F32, 5, 4, 3, 14u);
  set_f32(bad, 7, nan), set_f32(bad, 11, inf), set_f32(bad, 13, -inf), set_f32(bad, 59, nan);
  make_field(all_nan, CVR_SCALAR_F32, 5, 4, 3, 15u);
  for (size_t i = 0; i < 60; ++i) set_f32(all_nan, i, nan);

  const Cam oblique = camera(2.1f, 1.3f, -1.7f, -2.0f, -1.3f, 1.7f, 0.36f);
  const Cam inside = camera(0.1f, 0.1f, 0.2f, -0.4f, 0.7f, -0.85f, 1.0f);
  const Cam miss = camera(2.0f, 0.0f, 4.0f, 0.0f, 0.0f, -1.0f, 0.0f);  // a pencil beside the box
  const Cam wide = camera(0.1f, 0.1f, 0.2f, 0.0f, 0.0f, -1.0f, 1e30f);  // directions that overflow
  Cam broken = oblique;
  broken.iv[3] = nan;
  broken.iv[6] = inf;
  const uint32_t tiles[][4] = {{13, 7, 8, 8}, {19, 13, 8, 8}, {1, 1, 63, 47}, {64, 48, 0, 0}};

  // the value ranges of the four types' fields: f32 in [0, 1), u8, u16, i16
  const float top[4] = {1.0f, 255.0f, 65535.0f, 32767.0f}, bottom[4] = {0.0f, 0.0f, 0.0f, -32768.0f};
  std::vector<const Field*> fields;
  for (const Field& g : ragged) fields.push_back(&g);
  for (const Field* g : {&thin, &cube, &one, &bad, &all_nan}) fields.push_back(g);
  for (const Field* g : fields) {
    const uint32_t t = g->f.scalar_type;
    const float mid = bottom[t] + 0.6f * (top[t] - bottom[t]);
    for (uint32_t mode = 0; mode < 4; ++mode) {
      cvr_project_desc d = desc(mode, bottom[t], top[t], mid);
      for (const auto& tl : tiles) {
        const bool planes = tl[0] != 19;
        const bool bg = g == &all_nan;
        run(*g, oblique, tl[0], tl[1], tl[2], tl[3], d, planes, bg, "oblique");
        run(*g, inside, tl[0], tl[1], tl[2], tl[3], d, planes, bg, "inside");
        run(*g, miss, tl[0], tl[1], tl[2], tl[3], d, planes, true, "a miss is the background");
        if (tl[0] * tl[1] > 128u) continue;  // (a NaN chord marches max_steps: the small tiles only)
        run(*g, wide, tl[0], tl[1], tl[2], tl[3], d, planes, bg, "overflowing directions");
        run(*g, broken, tl[0], tl[1], tl[2], tl[3], d, planes, bg, "NaN and inf in the camera");
      }
      // other steps, a truncated march, no refinement and the most, a directional light, both ends of the exponent
      d.step = 0.125f, d.max_steps = 16u, d.refine = 0u, d.flags = 0u, d.light[0] = 0.3f, d.light[1] = 1.0f,
      d.light[2] = -0.4f, d.shininess_log2 = 10u;
      run(*g, oblique, 13, 7, 8, 8, d, true, g == &all_nan, "fine, truncated");
      d.step = 8.0f, d.max_steps = 65536u, d.refine = 8u, d.shininess_log2 = 0u;
      run(*g, inside, 13, 7, 8, 8, d, true, g == &all_nan, "coarse");
    }
    // an isosurface above the field misses everywhere; one at its bottom hits wherever there is a chord
    if (g != &bad && g != &all_nan) {
      run(*g, oblique, 19, 13, 8, 8, desc(CVR_PROJECT_ISO, 0.0f, 1.0f, top[t] + 1.0f), true, true, "iso above the field");
      run(*g, inside, 19, 13, 8, 8, desc(CVR_PROJECT_ISO, 0.0f, 1.0f, bottom[t]), true, false, "iso at the minimum");
    }
  }

  // the refusals reach no array
  std::vector<float> px(4, 0.0f);
  const Field& g = ragged[1];
  auto refused = [&](const cvr_field_desc& f, const cvr_project_desc& d, float* rgba, const char* what) {
    expect(cvr_field_project_host(&f, &d, oblique.iv, oblique.r2v, kFull, 1, 1, 0, 0, rgba, nullptr, nullptr) ==
               CVR_ERR_INVALID, what);
  };
  const cvr_project_desc ok = desc(CVR_PROJECT_ISO, 0.0f, 255.0f, 100.0f);
  expect(cvr_field_project_host(&g.f, nullptr, oblique.iv, oblique.r2v, kFull, 1, 1, 0, 0, px.data(), nullptr, nullptr) ==
             CVR_ERR_INVALID, "a NULL descriptor");
  cvr_field_desc f = g.f;
  f.res[1] = 0;
  refused(f, ok, px.data(), "a zero extent");
  f = g.f, f.res[0] = f.res[1] = f.res[2] = 2048u, f.scalar = nullptr;
  refused(f, ok, px.data(), "too many voxels");
  f = g.f, f.scalar_type = 4u;
  refused(f, ok, px.data(), "scalar_type");
  cvr_project_desc d = ok;
  d.mode = 4u;
  refused(g.f, d, px.data(), "mode");
  d = ok, d.box_max[1] = d.box_min[1];
  refused(g.f, d, px.data(), "an empty box");
  d = ok, d.step = 9.0f;
  refused(g.f, d, px.data(), "step");
  d = desc(CVR_PROJECT_MAX, 1.0f, 1.0f, 0.0f);
  refused(g.f, d, px.data(), "an empty window");
  d = ok, d.refine = 9u;
  refused(g.f, d, px.data(), "refine");
  d = ok, d.flags = 0u;
  refused(g.f, d, px.data(), "a zero light");
  d = ok, d.colour[2] = -1.0f;
  refused(g.f, d, px.data(), "a negative colour");
  refused(g.f, ok, nullptr, "a NULL image");
  refused(g.f, ok, px.data() + 1, "a misaligned image");
  if (failures) {
    fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  printf("project_host_check: ok\n");
  return 0;
}
