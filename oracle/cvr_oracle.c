/*
 * cvr_oracle.c - CPU ORACLE for the volumetric random walk.
 *
 * TEST INFRASTRUCTURE ONLY.  Only tests/, __graft_entry__.smoke() and the
 * cpu_baseline leg of bench.py may load this library; the product path
 * (cudavolumerenderer_amd/, libcvr.so) never links or calls it.
 *
 * What it is: a plain-C restatement of the reference's single-medium path
 * tracer hot path (Fe0437/CudaVolumeRenderer, implementation/src), one
 * function per reference function, each citing the file:line it follows.
 *
 * Parity status: PARTIALLY PINNED.
 *   - The reference cannot run here (CUDA-only, no nvcc/cuRAND; SURVEY.md
 *     §8(c)) and ships no tests or golden vectors, so the full walk is
 *     "parity unpinned" against the CUDA binary.
 *   - XORWOW's generator step is pinned against rocRAND's independent xorwow
 *     implementation (tests/test_oracle_rng.py); cuRAND's seeding constants
 *     and curand_uniform mapping are restated from the cuRAND headers (not
 *     verifiable in this container) -> unpinned.
 *   - The scene data paths (bucky raw loader transfer function, VDB reader)
 *     are pinned by fixtures (tests/golden, bonsai_small.vdb invariants).
 * Documented deviations from the CUDA binary:
 *   - libdevice transcendentals / rsqrtf are replaced by cvr_detmath.h so
 *     that the HIP kernels can be bit-exact with this oracle per path;
 *   - FMA contraction is explicit (det_fmaf) at the three hot-loop sites
 *     listed in DESIGN.md, everything else is uncontracted IEEE;
 *   - RNG is bound to path_id for every scheduler, except in
 *     oracle_render_thread_bound, which restates regenerationSK's own
 *     Rng(seed + tid) binding for lockstep threads (CVR_OPT_RNG_BINDING 1).
 */
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "cvr_detmath.h"

#define EXPORT __attribute__((visibility("default")))
#define EPS CVR_EPSILON_F

/* ------------------------------------------------------------ vectors --- */
typedef struct { float x, y, z; } f3;
static inline f3 mk3(float x, float y, float z) { f3 r = {x, y, z}; return r; }
static inline f3 add3(f3 a, f3 b) { return mk3(a.x + b.x, a.y + b.y, a.z + b.z); }
static inline f3 sub3(f3 a, f3 b) { return mk3(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline f3 mul3(f3 a, f3 b) { return mk3(a.x * b.x, a.y * b.y, a.z * b.z); }
static inline f3 div3(f3 a, f3 b) { return mk3(a.x / b.x, a.y / b.y, a.z / b.z); }
static inline f3 scl3(f3 a, float s) { return mk3(a.x * s, a.y * s, a.z * s); }
static inline f3 neg3(f3 a) { return mk3(-a.x, -a.y, -a.z); }
/* helper_math.h dot: a.x*b.x + a.y*b.y + a.z*b.z, left to right */
static inline float dot3(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static inline f3 cross3(f3 a, f3 b) {
  return mk3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
/* helper_math.h:1055 normalize = v*rsqrtf(dot(v,v)); restated as 1/sqrtf
 * (correctly rounded on both targets) - see header. */
static inline f3 normalize3(f3 v) { return scl3(v, 1.0f / det_sqrtf(dot3(v, v))); }

/* ---------------------------------------------------------------- RNG --- */
/* cuRAND XORWOW as used by Rng.h:22-30 (curand_init(seed,0,0),
 * curand_uniform).  Third-party (CUDA Toolkit 12.0, not vendored). */
typedef struct { uint32_t v[5]; uint32_t d; } xorwow_t;

/* The seeding structure (which scrambled seed words add / xor into which state
 * words, and the Weyl counter's start), with the generator's four scramble
 * constants as parameters: cuRAND's below; oracle_rng_state_consts runs it with
 * rocRAND's, whose xorwow_engine seeds with the same structure, so that structure
 * is pinned against an independent implementation (tests/test_oracle_cpu.py) and
 * only cuRAND's four constants are restated from the CUDA headers. */
static inline void rng_init_consts(xorwow_t* s, unsigned long long sd, uint32_t x0, uint32_t x1, uint32_t m0,
                                   uint32_t m1) {
  uint32_t s0 = ((uint32_t)sd) ^ x0;
  uint32_t s1 = ((uint32_t)(sd >> 32)) ^ x1;
  uint32_t t0 = m0 * s0;
  uint32_t t1 = m1 * s1;
  s->d = 6615241u + t1 + t0;
  s->v[0] = 123456789u + t0;
  s->v[1] = 362436069u ^ t0;
  s->v[2] = 521288629u + t1;
  s->v[3] = 88675123u ^ t1;
  s->v[4] = 5783321u + t0;
}
static inline void rng_init(xorwow_t* s, int32_t seed) {
  /* Rng(int seed) -> curand_init(unsigned long long): sign extension (Q3) */
  rng_init_consts(s, (unsigned long long)(long long)seed, 0xaad26b49u, 0xf7dcefddu, 1099087573u, 2591861531u);
}
static inline uint32_t rng_next(xorwow_t* s) {
  uint32_t t = s->v[0] ^ (s->v[0] >> 2);
  s->v[0] = s->v[1];
  s->v[1] = s->v[2];
  s->v[2] = s->v[3];
  s->v[3] = s->v[4];
  s->v[4] = (s->v[4] ^ (s->v[4] << 4)) ^ (t ^ (t << 1));
  s->d += 362437u;
  return s->v[4] + s->d;
}
/* curand_uniform: x * 2^-32 + 2^-33 in (0,1]; nvcc fuses to one FMA. */
static inline float rng_float(xorwow_t* s) {
  return det_fmaf((float)rng_next(s), 2.3283064e-10f, 1.1641532e-10f);
}

/* --------------------------------------------------------- scene data --- */
typedef struct {
  uint32_t res[3];
  const float* density; /* res.x*res.y*res.z, x fastest */
  const float* albedo;  /* float4 (rgb, w=1) per voxel */
  float box_min[3], box_max[3];
  float scale, max_density, g;
  float roughness[2];
  float eta; /* int_ior / ext_ior */
  /* Optional 8^3-leaf storage of the same grid (cvr_sparse_medium_desc
   * layout); when `leaves` is set, density/albedo are unused.  A storage
   * format only: texel values are those of the densified grid. */
  const uint32_t* leaves;
  uint32_t leaf_dims[3];
  const float* leaf_density;
  const float* leaf_albedo; /* NULL: albedo_bg everywhere */
  float albedo_bg[4];
} oracle_medium;

typedef struct {
  float inv_view[12];   /* c_inv_view_mat, 3 rows x float4 */
  float raster_to_view[2];
  float full_res[2];    /* c_pixel_index_range */
  float tile_res[2];    /* c_resolution */
  uint32_t offset[2];   /* c_offset */
  int32_t kernel;       /* 0 naiveSK, 2 regenerationSK, ... (Config.h Kernel) */
  uint32_t seed_base;   /* RNG seed = seed_base + path_id */
  uint32_t max_segments;/* safety cap (0 = none) */
  int32_t world_to_aabb;/* Q4: 0 the reference's p - min/extent, 1 fixed (CVR_OPT_WORLD_TO_AABB) */
} oracle_launch;

typedef struct {
  uint32_t image_id;
  uint32_t flags;       /* bit0 escaped (contributed), bit1 truncated */
  float T[3];
  uint32_t n_segments, n_steps, n_density, n_albedo;
} oracle_path;

typedef struct {
  uint64_t segments, steps, density, albedo, escaped, paths, truncated;
} oracle_stats;

/* ----------------------------------------------------- grid lookups ---- */
/* Volume.h:47-69 (MITSUBA_COMPARABLE manual trilinear) + texel rule of
 * RenderKernelLauncher.cu:20-25 / CudaVolPath.cpp:168-179: point-filtered,
 * clamp-addressed, unnormalised; the int index passes through uint, so -1
 * clamps to res-1 (Q5). */
static inline uint32_t texel(int i, uint32_t res) {
  uint32_t u = (uint32_t)i;
  return u < res - 1u ? u : res - 1u;
}
/* lerp convention shared with the kernels: fma(b, f, a*(1-f)) */
static inline float lerpf(float a, float b, float f, float fi) { return det_fmaf(b, f, a * fi); }

static inline float tex_density(const oracle_medium* m, uint32_t x, uint32_t y, uint32_t z) {
  if (m->leaves) {
    uint32_t slot = m->leaves[((size_t)(z >> 3) * m->leaf_dims[1] + (y >> 3)) * m->leaf_dims[0] + (x >> 3)];
    if (slot == 0xFFFFFFFFu) return 0.0f;
    return m->leaf_density[(size_t)slot * 512 + ((z & 7) * 8 + (y & 7)) * 8 + (x & 7)];
  }
  return m->density[((size_t)z * m->res[1] + y) * m->res[0] + x];
}
static inline float tex_albedo(const oracle_medium* m, uint32_t x, uint32_t y, uint32_t z, int c) {
  if (m->leaves) {
    uint32_t slot = m->leaves[((size_t)(z >> 3) * m->leaf_dims[1] + (y >> 3)) * m->leaf_dims[0] + (x >> 3)];
    if (slot == 0xFFFFFFFFu || !m->leaf_albedo) return m->albedo_bg[c];
    return m->leaf_albedo[((size_t)slot * 512 + ((z & 7) * 8 + (y & 7)) * 8 + (x & 7)) * 4 + c];
  }
  return m->albedo[(((size_t)z * m->res[1] + y) * m->res[0] + x) * 4 + c];
}

typedef struct { int x1, y1, z1; float fx, fy, fz; } tri_t;
/* DeviceVolume::volumeToGrid: p * (res - 1); g = (res - 1), or for the
 * density with the Q4 fix (res - 1)/extent (see woodcock) */
static inline tri_t tri_setup_g(f3 p, const float g[3]) {
  tri_t t;
  float cx = p.x * g[0];
  float cy = p.y * g[1];
  float cz = p.z * g[2];
  t.x1 = det_floor_i32(cx);
  t.y1 = det_floor_i32(cy);
  t.z1 = det_floor_i32(cz);
  t.fx = cx - (float)t.x1;
  t.fy = cy - (float)t.y1;
  t.fz = cz - (float)t.z1;
  return t;
}
static inline tri_t tri_setup(f3 p, const uint32_t res[3]) {
  const float g[3] = {(float)(res[0] - 1u), (float)(res[1] - 1u), (float)(res[2] - 1u)};
  return tri_setup_g(p, g);
}
static float density_lookup_g(const oracle_medium* m, f3 p, const float g[3]) {
  tri_t t = tri_setup_g(p, g);
  const uint32_t rx = m->res[0], ry = m->res[1], rz = m->res[2];
  uint32_t xa = texel(t.x1, rx), xb = texel(t.x1 + 1, rx);
  uint32_t ya = texel(t.y1, ry), yb = texel(t.y1 + 1, ry);
  uint32_t za = texel(t.z1, rz), zb = texel(t.z1 + 1, rz);
#define DV(x, y, z) tex_density(m, x, y, z)
  float d000 = DV(xa, ya, za), d001 = DV(xb, ya, za), d010 = DV(xa, yb, za), d011 = DV(xb, yb, za);
  float d100 = DV(xa, ya, zb), d101 = DV(xb, ya, zb), d110 = DV(xa, yb, zb), d111 = DV(xb, yb, zb);
#undef DV
  float _fx = 1.0f - t.fx, _fy = 1.0f - t.fy, _fz = 1.0f - t.fz;
  float a = lerpf(lerpf(d000, d001, t.fx, _fx), lerpf(d010, d011, t.fx, _fx), t.fy, _fy);
  float b = lerpf(lerpf(d100, d101, t.fx, _fx), lerpf(d110, d111, t.fx, _fx), t.fy, _fy);
  return lerpf(a, b, t.fz, _fz);
}
static float density_lookup(const oracle_medium* m, f3 p) {
  const float g[3] = {(float)(m->res[0] - 1u), (float)(m->res[1] - 1u), (float)(m->res[2] - 1u)};
  return density_lookup_g(m, p, g);
}
static f3 albedo_lookup(const oracle_medium* m, f3 p) {
  tri_t t = tri_setup(p, m->res);
  const uint32_t rx = m->res[0], ry = m->res[1], rz = m->res[2];
  uint32_t xa = texel(t.x1, rx), xb = texel(t.x1 + 1, rx);
  uint32_t ya = texel(t.y1, ry), yb = texel(t.y1 + 1, ry);
  uint32_t za = texel(t.z1, rz), zb = texel(t.z1 + 1, rz);
  float _fx = 1.0f - t.fx, _fy = 1.0f - t.fy, _fz = 1.0f - t.fz;
  float out[3];
  for (int c = 0; c < 3; ++c) {
#define AV(x, y, z) tex_albedo(m, x, y, z, c)
    float d000 = AV(xa, ya, za), d001 = AV(xb, ya, za), d010 = AV(xa, yb, za), d011 = AV(xb, yb, za);
    float d100 = AV(xa, ya, zb), d101 = AV(xb, ya, zb), d110 = AV(xa, yb, zb), d111 = AV(xb, yb, zb);
#undef AV
    float a = lerpf(lerpf(d000, d001, t.fx, _fx), lerpf(d010, d011, t.fx, _fx), t.fy, _fy);
    float b = lerpf(lerpf(d100, d101, t.fx, _fx), lerpf(d110, d111, t.fx, _fx), t.fy, _fy);
    out[c] = lerpf(a, b, t.fz, _fz);
  }
  return mk3(out[0], out[1], out[2]);
}

/* -------------------------------------------------------------- AABB --- */
typedef struct { float dist; f3 normal; int inside; } isect_t;

/* Geometry.h:55-92 (AABB::intersect).  The isect persists across segments of
 * one path: when no plane matches, the previous normal is kept. */
static int aabb_intersect(const oracle_medium* m, f3 o, f3 d, isect_t* is) {
  f3 bmin = mk3(m->box_min[0], m->box_min[1], m->box_min[2]);
  f3 bmax = mk3(m->box_max[0], m->box_max[1], m->box_max[2]);
  f3 invR = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
  f3 tbot = mul3(invR, sub3(bmin, o));
  f3 ttop = mul3(invR, sub3(bmax, o));
  f3 tmin = mk3(det_fminf(ttop.x, tbot.x), det_fminf(ttop.y, tbot.y), det_fminf(ttop.z, tbot.z));
  f3 tmax = mk3(det_fmaxf(ttop.x, tbot.x), det_fmaxf(ttop.y, tbot.y), det_fmaxf(ttop.z, tbot.z));
  float largest_tmin = det_fmaxf(det_fmaxf(tmin.x, tmin.y), det_fmaxf(tmin.x, tmin.z));
  float smallest_tmax = det_fminf(det_fminf(tmax.x, tmax.y), det_fminf(tmax.x, tmax.z));
  is->dist = (largest_tmin > EPS) ? largest_tmin : smallest_tmax;
  if (is->dist == ttop.x) is->normal = mk3(1, 0, 0);
  else if (is->dist == ttop.y) is->normal = mk3(0, 1, 0);
  else if (is->dist == ttop.z) is->normal = mk3(0, 0, 1);
  else if (is->dist == tbot.x) is->normal = mk3(-1, 0, 0);
  else if (is->dist == tbot.y) is->normal = mk3(0, -1, 0);
  else if (is->dist == tbot.z) is->normal = mk3(0, 0, -1);
  is->inside = dot3(is->normal, d) > 0.0f;
  return (smallest_tmax > largest_tmin) && (is->dist > 0.0f);
}

/* ------------------------------------------------------- Woodcock ------ */
/* Utilities.cuh:129-155 + Medium.h:135-143.  The density at a tentative
 * point beyond max_t is computed by the reference but never used (the loop
 * condition tests t <= max_t first), so it is not evaluated here.
 * worldToAABB (Utilities.cuh:129-132) is p - start/range by operator
 * precedence (Q4, the default).  fix_q4: the intended (p - start)/range, as
 * the kernels compute it with CVR_OPT_WORLD_TO_AABB 1: c = p - start, then the
 * grid coordinate c * ((res - 1)/range), one rounding per step. */
/* Evaluation log (oracle_trace_evals): one row per density evaluation of the
 * calling thread's walk, in walk order.  NULL outside that call, so every other
 * entry point pays one pointer test per evaluation. */
typedef struct {
  uint32_t path_id;
  float cx, cy, cz; /* the grid coordinate tri_setup_g computes (c * g) */
  float xi_test;    /* the test draw */
  float test_value; /* fl(fl(scale * rho) * inv) */
} oracle_eval;
typedef struct {
  oracle_eval* rows;
  uint64_t cap, n; /* n counts every evaluation; rows beyond cap are not written */
  uint32_t path_id;
} eval_log_t;
static __thread eval_log_t* tl_eval_log = NULL;

static float woodcock(const oracle_medium* m, f3 o, f3 d, float max_t, xorwow_t* rng,
                      uint32_t* n_steps, uint32_t* n_density, int fix_q4) {
  f3 bmin = mk3(m->box_min[0], m->box_min[1], m->box_min[2]);
  f3 ext = sub3(mk3(m->box_max[0], m->box_max[1], m->box_max[2]), bmin);
  f3 shift = fix_q4 ? bmin : div3(bmin, ext); /* worldToAABB: p - start/range (Q4) */
  float g[3] = {(float)(m->res[0] - 1u), (float)(m->res[1] - 1u), (float)(m->res[2] - 1u)};
  if (fix_q4) {
    g[0] = g[0] / ext.x;
    g[1] = g[1] / ext.y;
    g[2] = g[2] / ext.z;
  }
  float inv = 1.0f / (m->scale * m->max_density);
  float t = 0.0f;
  for (;;) {
    float xi = rng_float(rng);
    t = det_fmaf(-det_logf(det_fmaxf(xi, EPS)), inv, t); /* woodcockStep */
    ++*n_steps;
    if (!(t <= max_t)) break;
    f3 p = mk3(det_fmaf(t, d.x, o.x), det_fmaf(t, d.y, o.y), det_fmaf(t, d.z, o.z));
    f3 c = sub3(p, shift);
    float rho = m->scale * density_lookup_g(m, c, g);
    ++*n_density;
    const float xt = rng_float(rng);
    const float tv = rho * inv;
    if (tl_eval_log) {
      eval_log_t* lg = tl_eval_log;
      if (lg->n < lg->cap) {
        oracle_eval* e = &lg->rows[lg->n];
        e->path_id = lg->path_id;
        e->cx = c.x * g[0];
        e->cy = c.y * g[1];
        e->cz = c.z * g[2];
        e->xi_test = xt;
        e->test_value = tv;
      }
      ++lg->n;
    }
    if (!(tv < xt)) break;
  }
  return t;
}

/* ------------------------------------------------------------ phase ---- */
/* HG.h:11-63 (generateLocalBasis, sphericalDirection, ImportanceSampleHG) */
static f3 hg_sample(f3 v, float g, float e1, float e2) {
  float cosT;
  if (det_fabsf(g) > EPS) {
    float sq = (1.0f - g * g) / ((1.0f - g) + (2.0f * g) * e1);
    cosT = ((1.0f + g * g) - sq * sq) / (2.0f * det_fabsf(g));
  } else {
    cosT = 1.0f - 2.0f * e1;
  }
  float sinT = det_sqrtf(det_fmaxf(0.0f, 1.0f - cosT * cosT));
  float phi = CVR_TWOPI_F * e2;
  float invN = 1.0f / det_sqrtf(v.x * v.x + v.z * v.z);
  f3 v1 = mk3(v.z * invN, 0.0f, (-v.x) * invN);
  f3 v2 = cross3(v, v1);
  float sp, cp;
  det_sincosf(phi, &sp, &cp);
  return add3(add3(scl3(v1, sinT * cp), scl3(v2, sinT * sp)), scl3(v, cosT));
}

/* ------------------------------------------------------------- GGX ----- */
/* GGX.h:13-38 */
static float fresnel_dielectric(float eta, float ndotwi, float* ndotwt) {
  if (eta == 1.0f) { *ndotwt = -ndotwi; return 0.0f; }
  float scale = (ndotwi > 0.0f) ? 1.0f / eta : eta;
  float sin_sqr = 1.0f - ndotwi * ndotwi;
  float ndotwt_sqr = 1.0f - (sin_sqr * scale) * scale;
  if (ndotwt_sqr <= 0.0f) { *ndotwt = 0.0f; return 1.0f; }
  float a_wi = det_fabsf(ndotwi);
  float a_wt = det_sqrtf(ndotwt_sqr);
  float Rs = (a_wi - eta * a_wt) / (a_wi + eta * a_wt);
  float Rp = (eta * a_wi - a_wt) / (eta * a_wi + a_wt);
  *ndotwt = (ndotwi > 0.0f) ? -a_wt : a_wt;
  return 0.5f * (Rs * Rs + Rp * Rp);
}
/* GGX.h:85-144 */
static void sample_visible11(float thetaI, float sx, float sy, float* ox, float* oy) {
  float phi = (2.0f * CVR_PI_F) * sy;
  if (thetaI < 1e-4f) {
    float r = det_sqrtf(det_fmaxf(0.0f, sx / (1.0f - sx)));
    float sp, cp;
    det_sincosf(phi, &sp, &cp);
    *ox = r * cp;
    *oy = r * sp;
    return;
  }
  float tanThetaI = det_tanf(thetaI);
  float a = 1.0f / tanThetaI;
  a = 1.0f + (1.0f / (a * a));
  float G1 = 2.0f / (1.0f + det_sqrtf(a));
  float A = ((2.0f * sx) / G1) - 1.0f;
  if (det_fabsf(A) == 1.0f) A -= (A < 0.0f ? -1.0f : 1.0f) * EPS;
  float tmp = 1.0f / (A * A - 1.0f);
  float B = tanThetaI;
  float D = det_sqrtf(det_fmaxf(0.0f, ((B * B) * tmp) * tmp - (A * A - B * B) * tmp));
  float s1 = B * tmp - D, s2 = B * tmp + D;
  float slope_x = (A < 0.0f || s2 > 1.0f / tanThetaI) ? s1 : s2;
  float S;
  if (sy > 0.5f) { S = 1.0f; sy = 2.0f * (sy - 0.5f); }
  else { S = -1.0f; sy = 2.0f * (0.5f - sy); }
  float z = (sy * (sy * (sy * (-0.365728915865723f) + 0.790235037209296f) - 0.424965825137544f) +
             0.000152998850436920f) /
            (sy * (sy * (sy * (sy * 0.169507819808272f - 0.397203533833404f) - 0.232500544458471f) +
                   1.0f) -
             0.539825872510702f);
  *ox = slope_x;
  *oy = (S * z) * det_sqrtf(1.0f + slope_x * slope_x);
}
/* GGX.h:146-181 */
static f3 ggx_sample_vndf(f3 wi_, float ax, float ay, float sx, float sy) {
  f3 wi = normalize3(mk3(ax * wi_.x, ay * wi_.y, wi_.z));
  float theta = 0.0f, phi = 0.0f;
  if (wi.z < 0.999999f) {
    theta = det_acosf(wi.z);
    phi = det_atan2f(wi.y, wi.x);
  }
  float sinPhi, cosPhi;
  det_sincosf(phi, &sinPhi, &cosPhi);
  float slx, sly;
  sample_visible11(theta, sx, sy, &slx, &sly);
  float rx = cosPhi * slx - sinPhi * sly;
  float ry = sinPhi * slx + cosPhi * sly;
  rx *= ax;
  ry *= ay;
  float n = 1.0f / det_sqrtf(rx * rx + ry * ry + 1.0f);
  return mk3(-rx * n, -ry * n, n);
}
/* GGX.h:213-255 */
static float project_roughness(f3 v, float ax, float ay) {
  float invSinTheta2 = 1.0f / (1.0f - v.z * v.z);
  if (ax == ay || invSinTheta2 <= 0.0f) return ax;
  float cosPhi2 = v.x * v.x * invSinTheta2;
  float sinPhi2 = v.y * v.y * invSinTheta2;
  return det_sqrtf(cosPhi2 * ax * ax + sinPhi2 * ay * ay);
}
static float ggx_g1(float ax, float ay, f3 v, f3 m) {
  if (dot3(v, m) * v.z <= 0.0f) return 0.0f;
  float temp = 1.0f - v.z * v.z;
  if (temp <= 0.0f) return 0.0f;
  float tn = det_fabsf(det_sqrtf(temp) / v.z);
  if (tn == 0.0f) return 1.0f;
  float root = project_roughness(v, ax, ay) * tn;
  return 2.0f / (1.0f + det_sqrtf(1.0f + root * root));
}
/* GGX.h:265-326.  wo aliases the path direction (Bsdf.h:352-357 passes
 * path.ray.d as output_dir): a failed sample may still have overwritten it
 * (Q8). */
static int ggx_sample(const oracle_medium* m, f3 wi, xorwow_t* rng, f3* wo, float* weight) {
  float ndotwi = wi.z;
  if (ndotwi == 0.0f) { *weight = 0.0f; return 0; }
  *weight = 1.0f;
  float sign = wi.z / det_fabsf(wi.z);
  float s0 = rng_float(rng);
  float s1 = rng_float(rng);
  f3 wh = ggx_sample_vndf(scl3(wi, sign), m->roughness[0], m->roughness[1], s0, s1);
  float whdotwt = __builtin_nanf("");
  float whdotwi = dot3(wh, wi);
  float F = fresnel_dielectric(m->eta, whdotwi, &whdotwt);
  if (rng_float(rng) <= F) {
    *wo = sub3(scl3(wh, 2.0f * whdotwi), wi); /* reflect */
    if (wi.z * wo->z <= 0.0f) { *weight = 0.0f; return 0; }
  } else {
    if (whdotwt == 0.0f) { *weight = 0.0f; return 0; }
    float eta = m->eta;
    if (whdotwt < 0.0f) eta = 1.0f / eta; /* refract */
    *wo = sub3(scl3(wh, whdotwi * eta + whdotwt), scl3(wi, eta));
    if (wi.z * wo->z >= 0.0f) { *weight = 0.0f; return 0; }
  }
  *weight *= ggx_g1(m->roughness[0], m->roughness[1], *wo, wh);
  return 1;
}

/* ----------------------------------------------------------- frame ----- */
/* CVRMath.h:58-91 */
typedef struct { f3 x, y, z; } frame_t;
static frame_t frame_from_z(f3 n) {
  frame_t f;
  f.z = normalize3(n);
  f3 tx = (det_fabsf(f.z.x) > 0.99f) ? mk3(0, 1, 0) : mk3(1, 0, 0);
  f.y = normalize3(cross3(f.z, tx));
  f.x = cross3(f.y, f.z);
  return f;
}
static f3 frame_to_local(const frame_t* f, f3 a) { return mk3(dot3(a, f->x), dot3(a, f->y), dot3(a, f->z)); }
static f3 frame_to_world(const frame_t* f, f3 a) {
  return add3(add3(scl3(f->x, a.x), scl3(f->y, a.y)), scl3(f->z, a.z));
}

/* ---------------------------------------------------------- camera ----- */
/* Utilities.cuh:180-213 + CVRMath.h:19-39 */
static void camera_ray(const oracle_launch* L, float px, float py, xorwow_t* rng, f3* o, f3* d) {
  float r0 = rng_float(rng);
  float r1 = rng_float(rng);
  float rx = ((px + r0) * 2.0f) / L->full_res[0] - 1.0f;
  float ry = ((py + r1) * 2.0f) / L->full_res[1] - 1.0f;
  rx = L->raster_to_view[0] * rx;
  ry = L->raster_to_view[1] * ry;
  const float* M = L->inv_view;
  /* mul(float3x4, float4(0,0,0,1)): float4 dot, left to right */
  *o = mk3(0.0f * M[0] + 0.0f * M[1] + 0.0f * M[2] + 1.0f * M[3],
           0.0f * M[4] + 0.0f * M[5] + 0.0f * M[6] + 1.0f * M[7],
           0.0f * M[8] + 0.0f * M[9] + 0.0f * M[10] + 1.0f * M[11]);
  f3 v = normalize3(mk3(rx, ry, 1.0f));
  *d = mk3(dot3(v, mk3(M[0], M[1], M[2])), dot3(v, mk3(M[4], M[5], M[6])),
           dot3(v, mk3(M[8], M[9], M[10])));
}

/* ------------------------------------------------------------ naiveMK -- */
/* utilhash / makeSeededRng (Utilities.cuh:157-178): the naiveMK RNG is
 * re-seeded from (iteration, pixel, depth) at every kernel launch. */
static uint32_t utilhash(uint32_t a) {
  a = (a + 0x7ed55d16u) + (a << 12);
  a = (a ^ 0xc761c23cu) ^ (a >> 19);
  a = (a + 0x165667b1u) + (a << 5);
  a = (a + 0xd3a2646cu) ^ (a << 9);
  a = (a + 0xfd7046c5u) + (a << 3);
  a = (a ^ 0xb55a4f09u) ^ (a >> 16);
  return a;
}
static void rng_seeded(xorwow_t* s, uint32_t iteration, uint32_t index, uint32_t depth) {
  const uint32_t h = utilhash(0x80000000u | (depth << 22) | iteration) ^ utilhash(index);
  rng_init(s, (int32_t)h); /* Rng(int) */
}

/* NaiveVolPTmk_kernel::d_init (NaiveVolPTmk_kernel.cuh:20-77): camera ray
 * from the (iteration, pixel, 0) stream, AABB test (a miss adds (1,1,1) to
 * the pixel), GGX at the box before any medium test (Q12; a failed sample
 * drops the path).  Returns 0 alive, 1 missed, 2 dropped. */
typedef struct { f3 o, d, T; } mk_path_t;
static int mk_init(const oracle_medium* m, const oracle_launch* L, uint32_t iteration, uint32_t image_id,
                   mk_path_t* p) {
  xorwow_t rng;
  rng_seeded(&rng, iteration, image_id, 0u);
  float px = (float)(image_id % (uint32_t)L->tile_res[0]) + (float)L->offset[0];
  float py = det_floorf((float)image_id / L->tile_res[0]) + (float)L->offset[1];
  camera_ray(L, px, py, &rng, &p->o, &p->d);
  p->T = mk3(1.0f, 1.0f, 1.0f);
  isect_t is;
  is.dist = 0.0f;
  is.normal = mk3(0, 0, 0);
  is.inside = 0;
  if (!aabb_intersect(m, p->o, p->d, &is)) return 1;
  if (is.dist < 0.0f) is.dist = 0.0f; /* clamp to near plane */
  p->o = add3(p->o, scl3(p->d, is.dist));
  frame_t fr = frame_from_z(is.normal);
  f3 dir = frame_to_local(&fr, normalize3(neg3(p->d)));
  float weight = 1.0f;
  if (!ggx_sample(m, dir, &rng, &p->d, &weight)) return 2;
  p->T = scl3(p->T, weight);
  p->d = frame_to_world(&fr, p->d);
  p->o = add3(p->o, scl3(p->d, EPS));
  return 0;
}

/* One NaiveVolPTmk_kernel::d_extend bounce (NaiveVolPTmk_kernel.cuh:79-151):
 * re-seed from (iteration, pixel, depth), three unused draws (Q12), one
 * naiveSK segment (scatter with -eps), roulette.  Returns 0 alive,
 * 3 escaped (contributes T), 4 died in roulette. */
static int mk_extend(const oracle_medium* m, const oracle_launch* L, uint32_t iteration, uint32_t image_id,
                     uint32_t depth, mk_path_t* p, oracle_path* res) {
  xorwow_t rng;
  rng_seeded(&rng, iteration, image_id, depth);
  (void)rng_float(&rng); /* float3 e = rng.getFloat3(), unused */
  (void)rng_float(&rng);
  (void)rng_float(&rng);
  isect_t is;
  is.dist = 0.0f; /* a fresh SimpleIsect per d_extend */
  is.normal = mk3(0, 0, 0);
  is.inside = 0;
  if (!aabb_intersect(m, p->o, p->d, &is)) return 3;
  float sampled = 0.0f;
  int collided = 0;
  if (is.inside) {
    sampled = woodcock(m, p->o, p->d, is.dist, &rng, &res->n_steps, &res->n_density, L->world_to_aabb);
    collided = sampled < is.dist;
  }
  if (!collided) {
    frame_t fr = frame_from_z(is.normal);
    f3 dir = frame_to_local(&fr, normalize3(neg3(p->d)));
    p->o = add3(p->o, scl3(p->d, is.dist));
    float weight = 1.0f;
    if (ggx_sample(m, dir, &rng, &p->d, &weight)) {
      p->T = scl3(p->T, weight);
      p->d = frame_to_world(&fr, p->d);
      p->o = add3(p->o, scl3(p->d, EPS));
    }
  } else {
    p->o = sub3(add3(p->o, scl3(p->d, sampled)), scl3(p->d, EPS));
    f3 bmin = mk3(m->box_min[0], m->box_min[1], m->box_min[2]);
    f3 bmax = mk3(m->box_max[0], m->box_max[1], m->box_max[2]);
    f3 a = albedo_lookup(m, div3(sub3(p->o, bmin), sub3(bmax, bmin)));
    ++res->n_albedo;
    p->T = mul3(p->T, a);
    float e1 = rng_float(&rng);
    float e2 = rng_float(&rng);
    p->d = hg_sample(p->d, m->g, e1, e2);
  }
  float q = det_fminf(1.0f, det_fmaxf(det_fmaxf(p->T.x, p->T.y), p->T.z));
  if (rng_float(&rng) > q) return 4;
  p->T = mk3(p->T.x / q, p->T.y / q, p->T.z / q);
  return 0;
}

/* NaiveVolPTmk_kernel.cuh:20-151 + NaiveVolPTmk::launchRender/extend
 * (RenderKernelLauncher.cu:183-272).  Path id = iteration * tile_px + pixel,
 * as for the other kernels.  Each bounce (d_extend) re-seeds, so per path the
 * launches reduce to d_init + d_extend(depth = 0, 1, ...) until the path
 * ends.  Compaction keeps every live path (Q11 fixed: the reference's
 * `end - begin - 1` drops one live path per bounce, restated by
 * oracle_render_mk_reference).  Flags: bit0 contributed (T), bit1 truncated,
 * bit2 missed the box at init (T = 1), bit3 dropped by a failed GGX sample at
 * init.  n_segments counts d_init plus every d_extend. */
static void trace_path_mk(const oracle_medium* m, const oracle_launch* L, uint32_t path_id, oracle_path* res) {
  const uint32_t tile_px = (uint32_t)(L->tile_res[0] * L->tile_res[1]);
  const uint32_t image_id = path_id % tile_px;
  const uint32_t iteration = path_id / tile_px;
  mk_path_t p;
  memset(res, 0, sizeof(*res));
  res->image_id = image_id;
  res->n_segments = 1;
  const int s0 = mk_init(m, L, iteration, image_id, &p);
  if (s0 == 1) {
    res->flags = 1u | 4u;
    res->T[0] = res->T[1] = res->T[2] = 1.0f;
    return;
  }
  if (s0 == 2) {
    res->flags = 8u;
    return;
  }
  for (uint32_t depth = 0;; ++depth) {
    if (L->max_segments && res->n_segments >= L->max_segments) { res->flags |= 2u; break; }
    ++res->n_segments;
    const int e = mk_extend(m, L, iteration, image_id, depth, &p, res);
    if (e == 3) res->flags |= 1u;
    if (e != 0) break;
  }
  res->T[0] = p.T.x;
  res->T[1] = p.T.y;
  res->T[2] = p.T.z;
}

/* naiveMK with the reference's compaction count (quirk Q11 reproduced,
 * CVR_OPT_MK_COMPACTION 1): NaiveVolPTmk::launchRender/extend
 * (RenderKernelLauncher.cu:183-272) over `iterations` passes of the tile.
 * The active list starts as the pixel ids in order (d_init writes
 * active[img] = img or -1) and thrust::remove_if compacts it stably, so it
 * stays in ascending pixel order; after each bounce the processed count is
 * (live paths) - 1: the live path with the highest pixel id is never extended
 * again.  A bounce that leaves no live path underflows the reference's uint
 * count (its next launch reads stale entries): returns -2 with the iteration
 * and bounce in err[0..1].  `out` is the tile accumulator. */
EXPORT int oracle_render_mk_reference(const oracle_medium* m, const oracle_launch* L, uint32_t iterations,
                                      float* out, oracle_stats* stats, uint32_t err[2]) {
  const uint32_t tile_px = (uint32_t)(L->tile_res[0] * L->tile_res[1]);
  mk_path_t* st = (mk_path_t*)calloc(tile_px ? tile_px : 1, sizeof(mk_path_t));
  uint8_t* live = (uint8_t*)calloc(tile_px ? tile_px : 1, 1);
  if (!st || !live) return -1;
  oracle_stats sa;
  memset(&sa, 0, sizeof(sa));
  int rc = 0;
  for (uint32_t it = 0; it < iterations && rc == 0; ++it) {
    for (uint32_t img = 0; img < tile_px; ++img) {
      const int s0 = mk_init(m, L, it, img, &st[img]);
      sa.paths++;
      sa.segments++;
      live[img] = s0 == 0;
      if (s0 == 1) { /* d_output[img_id] += (1,1,1,1) */
        out[4 * (size_t)img + 0] += 1.0f;
        out[4 * (size_t)img + 1] += 1.0f;
        out[4 * (size_t)img + 2] += 1.0f;
        out[4 * (size_t)img + 3] = 1.0f;
        sa.escaped++;
      }
    }
    uint64_t n_processed = tile_px;
    for (uint32_t depth = 0; n_processed != 0; ++depth) {
      uint32_t count = 0, max_id = 0;
      for (uint32_t img = 0; img < tile_px; ++img) {
        if (!live[img]) continue;
        oracle_path r;
        memset(&r, 0, sizeof(r));
        const int e = mk_extend(m, L, it, img, depth, &st[img], &r);
        sa.segments++;
        sa.steps += r.n_steps;
        sa.density += r.n_density;
        sa.albedo += r.n_albedo;
        if (e == 3) {
          out[4 * (size_t)img + 0] += st[img].T.x;
          out[4 * (size_t)img + 1] += st[img].T.y;
          out[4 * (size_t)img + 2] += st[img].T.z;
          out[4 * (size_t)img + 3] = 1.0f;
          sa.escaped++;
        }
        if (e == 0) {
          ++count;
          max_id = img;
        } else {
          live[img] = 0;
        }
      }
      if (count == 0) {
        if (err) {
          err[0] = it;
          err[1] = depth;
        }
        rc = -2;
        break;
      }
      n_processed = count - 1u;
      live[max_id] = 0; /* the compacted list's last entry, dropped by end - begin - 1 */
    }
  }
  free(st);
  free(live);
  if (stats) *stats = sa;
  return rc;
}

/* ----------------------------------------------------------- path ------ */
/* NaiveVolPTsk_kernel.cuh:17-87 (kernel 0) and
 * RegenerationVolPTsk_kernel.cuh:146-232 (kernel 2, no -eps at scatter, Q6).
 * `out` (optional) is the tile accumulator (float4 per pixel). */
EXPORT void oracle_trace_path(const oracle_medium* m, const oracle_launch* L, uint32_t path_id,
                              oracle_path* res) {
  if (L->kernel == 1) {
    trace_path_mk(m, L, path_id, res);
    return;
  }
  const uint32_t tile_px = (uint32_t)(L->tile_res[0] * L->tile_res[1]);
  const uint32_t image_id = path_id % tile_px;
  xorwow_t rng;
  rng_init(&rng, (int32_t)(L->seed_base + path_id));
  float px = (float)(image_id % (uint32_t)L->tile_res[0]) + (float)L->offset[0];
  float py = det_floorf((float)image_id / L->tile_res[0]) + (float)L->offset[1];
  f3 o, d;
  camera_ray(L, px, py, &rng, &o, &d);
  f3 T = mk3(1.0f, 1.0f, 1.0f);
  isect_t is;
  is.dist = 0.0f;
  is.normal = mk3(0, 0, 0);
  is.inside = 0;
  const int scatter_eps = (L->kernel != 2);
  memset(res, 0, sizeof(*res));
  res->image_id = image_id;
  for (;;) {
    if (L->max_segments && res->n_segments >= L->max_segments) { res->flags |= 2u; break; }
    ++res->n_segments;
    if (!aabb_intersect(m, o, d, &is)) {
      res->flags |= 1u; /* atomicVectorAdd(T * Le), Le = 1 */
      break;
    }
    float sampled = 0.0f;
    int collided = 0;
    if (is.inside) {
      sampled = woodcock(m, o, d, is.dist, &rng, &res->n_steps, &res->n_density, L->world_to_aabb);
      collided = sampled < is.dist;
    }
    if (!collided) {
      frame_t fr = frame_from_z(is.normal);
      f3 dir = frame_to_local(&fr, normalize3(neg3(d)));
      o = add3(o, scl3(d, is.dist));
      float weight = 1.0f;
      if (ggx_sample(m, dir, &rng, &d, &weight)) {
        T = scl3(T, weight);
        d = frame_to_world(&fr, d);
        o = add3(o, scl3(d, EPS));
      }
    } else {
      o = add3(o, scl3(d, sampled));
      if (scatter_eps) o = sub3(o, scl3(d, EPS));
      f3 bmin = mk3(m->box_min[0], m->box_min[1], m->box_min[2]);
      f3 bmax = mk3(m->box_max[0], m->box_max[1], m->box_max[2]);
      f3 a = albedo_lookup(m, div3(sub3(o, bmin), sub3(bmax, bmin)));
      ++res->n_albedo;
      T = mul3(T, a);
      float e1 = rng_float(&rng);
      float e2 = rng_float(&rng);
      d = hg_sample(d, m->g, e1, e2);
    }
    /* Russian roulette, NaiveVolPTsk_kernel.cuh:75-84 (always draws, Q9) */
    float p = det_fminf(1.0f, det_fmaxf(det_fmaxf(T.x, T.y), T.z));
    if (rng_float(&rng) > p) break;
    T = mk3(T.x / p, T.y / p, T.z / p);
  }
  res->T[0] = T.x;
  res->T[1] = T.y;
  res->T[2] = T.z;
}

/* Per-path records for path ids [first, first+count) (debug parity). */
EXPORT void oracle_trace_paths(const oracle_medium* m, const oracle_launch* L, uint32_t first,
                               uint32_t count, oracle_path* out) {
  for (uint32_t i = 0; i < count; ++i) oracle_trace_path(m, L, first + i, &out[i]);
}

/* oracle_trace_paths plus the evaluation log: `evals` receives the first `cap`
 * density evaluations of path ids [first, first+count) in walk order (every
 * kernel id: the log is written by woodcock()); returns how many there were, so
 * a call with cap 0 sizes the buffer.  Single-threaded. */
EXPORT uint64_t oracle_trace_evals(const oracle_medium* m, const oracle_launch* L, uint32_t first,
                                   uint32_t count, oracle_path* out, oracle_eval* evals, uint64_t cap) {
  eval_log_t lg;
  lg.rows = evals;
  lg.cap = evals ? cap : 0;
  lg.n = 0;
  tl_eval_log = &lg;
  for (uint32_t i = 0; i < count; ++i) {
    lg.path_id = first + i;
    oracle_trace_path(m, L, first + i, &out[i]);
  }
  tl_eval_log = NULL;
  return lg.n;
}

/* ---------------------------------------------------- tile render ------ */
typedef struct {
  const oracle_medium* m;
  const oracle_launch* L;
  uint64_t first, stride, count;
  float* accum; /* private tile accumulator, float4 */
  oracle_stats st;
} job_t;

static void* render_job(void* arg) {
  job_t* j = (job_t*)arg;
  oracle_path r;
  for (uint64_t i = 0; i < j->count; ++i) {
    uint32_t pid = (uint32_t)(j->first + i * j->stride);
    oracle_trace_path(j->m, j->L, pid, &r);
    j->st.paths++;
    j->st.segments += r.n_segments;
    j->st.steps += r.n_steps;
    j->st.density += r.n_density;
    j->st.albedo += r.n_albedo;
    if (r.flags & 2u) j->st.truncated++;
    if (r.flags & 1u) {
      float* px = j->accum + 4 * (size_t)r.image_id;
      px[0] += r.T[0];
      px[1] += r.T[1];
      px[2] += r.T[2];
      px[3] = 1.0f;
      j->st.escaped++;
    }
  }
  return NULL;
}

/* Render path ids first + k*stride, k in [0,count), into the tile buffer
 * `out` (tile_w*tile_h float4, accumulated into).  With nthreads>1 each
 * thread accumulates a contiguous share of k privately; shares are summed in
 * thread order, so the result is deterministic for a given nthreads. */
EXPORT int oracle_render(const oracle_medium* m, const oracle_launch* L, uint64_t first,
                         uint64_t stride, uint64_t count, float* out, int nthreads,
                         oracle_stats* stats) {
  if (nthreads < 1) nthreads = 1;
  const size_t npx = (size_t)(uint32_t)(L->tile_res[0] * L->tile_res[1]);
  job_t* jobs = (job_t*)calloc((size_t)nthreads, sizeof(job_t));
  pthread_t* th = (pthread_t*)calloc((size_t)nthreads, sizeof(pthread_t));
  if (!jobs || !th) return -1;
  uint64_t per = count / (uint64_t)nthreads, rem = count % (uint64_t)nthreads, at = 0;
  for (int t = 0; t < nthreads; ++t) {
    uint64_t c = per + ((uint64_t)t < rem ? 1 : 0);
    jobs[t].m = m;
    jobs[t].L = L;
    jobs[t].first = first + at * stride;
    jobs[t].stride = stride;
    jobs[t].count = c;
    jobs[t].accum = (t == 0) ? out : (float*)calloc(npx * 4, sizeof(float));
    at += c;
  }
  for (int t = 1; t < nthreads; ++t) pthread_create(&th[t], NULL, render_job, &jobs[t]);
  render_job(&jobs[0]);
  for (int t = 1; t < nthreads; ++t) pthread_join(th[t], NULL);
  oracle_stats st;
  memset(&st, 0, sizeof(st));
  for (int t = 0; t < nthreads; ++t) {
    if (t > 0) {
      for (size_t i = 0; i < npx; ++i) {
        out[4 * i + 0] += jobs[t].accum[4 * i + 0];
        out[4 * i + 1] += jobs[t].accum[4 * i + 1];
        out[4 * i + 2] += jobs[t].accum[4 * i + 2];
        if (jobs[t].accum[4 * i + 3] != 0.0f) out[4 * i + 3] = 1.0f;
      }
      free(jobs[t].accum);
    }
    st.segments += jobs[t].st.segments;
    st.steps += jobs[t].st.steps;
    st.density += jobs[t].st.density;
    st.albedo += jobs[t].st.albedo;
    st.escaped += jobs[t].st.escaped;
    st.paths += jobs[t].st.paths;
    st.truncated += jobs[t].st.truncated;
  }
  if (stats) *stats = st;
  free(jobs);
  free(th);
  return 0;
}

/* ---------------------------------------- thread-bound regenerationSK -- */
/* RegenerationVolPTsk_kernel::d_render_single_thread_regeneration
 * (RegenerationVolPTsk_kernel.cuh:146-232) with the RNG bound to the
 * persistent THREAD, not the path (CVR_OPT_RNG_BINDING = 1):
 *   - thread tid owns one stream, Rng(seed + tid) (:156), for every path it
 *     takes;
 *   - one loop iteration = [take a path if idle] + one segment + roulette;
 *     the roulette block runs after an escape too (:220-229), so an escaping
 *     path draws one more number from the thread's stream;
 *   - the SimpleIsect lives across the thread's paths (:155): a segment whose
 *     distance matches no box plane keeps the previous path's normal.
 * The reference takes path ids with one atomicAdd per idle thread, in an
 * order the hardware picks.  Restated here for `n_threads` threads advancing
 * in lockstep, idle threads taking consecutive ids in thread order at the top
 * of each iteration: the order a single 64-lane wave produces with one
 * wave-aggregated atomic (k_regen_thread launched as one wave), so that
 * launch is deterministic and comparable path by path.  Path ids are
 * first + [0, count); `out` is the tile accumulator (float4 per pixel). */
typedef struct {
  xorwow_t rng;
  isect_t is;
  f3 o, d, T;
  uint32_t image_id, nseg;
  int active, done;
} tb_thread_t;

EXPORT int oracle_render_thread_bound(const oracle_medium* m, const oracle_launch* L, uint32_t n_threads,
                                      uint32_t first, uint32_t count, float* out, oracle_stats* stats) {
  if (n_threads == 0) return -1;
  tb_thread_t* th = (tb_thread_t*)calloc(n_threads, sizeof(tb_thread_t));
  if (!th) return -1;
  oracle_stats st;
  memset(&st, 0, sizeof(st));
  const uint32_t tile_px = (uint32_t)(L->tile_res[0] * L->tile_res[1]);
  for (uint32_t t = 0; t < n_threads; ++t) {
    rng_init(&th[t].rng, (int32_t)(L->seed_base + t)); /* Rng(seed + tid): int, sign-extended (Q3) */
    th[t].is.dist = 0.0f;
    th[t].is.normal = mk3(0, 0, 0);
    th[t].is.inside = 0;
  }
  uint32_t head = 0, live = n_threads;
  while (live) {
    /* regenerate (:160-180): idle threads take ids in thread order */
    for (uint32_t t = 0; t < n_threads; ++t) {
      tb_thread_t* p = &th[t];
      if (p->done || p->active) continue;
      if (head >= count) {
        p->done = 1;
        --live;
        continue;
      }
      const uint32_t path_id = first + head++;
      p->image_id = path_id % tile_px;
      float px = (float)(p->image_id % (uint32_t)L->tile_res[0]) + (float)L->offset[0];
      float py = det_floorf((float)p->image_id / L->tile_res[0]) + (float)L->offset[1];
      camera_ray(L, px, py, &p->rng, &p->o, &p->d);
      p->T = mk3(1.0f, 1.0f, 1.0f);
      p->nseg = 0;
      p->active = 1;
      st.paths++;
    }
    for (uint32_t t = 0; t < n_threads; ++t) {
      tb_thread_t* p = &th[t];
      if (!p->active) continue;
      if (L->max_segments && p->nseg >= L->max_segments) { /* safety cap, as the path-bound walk */
        st.truncated++;
        p->active = 0;
        continue;
      }
      p->nseg++;
      st.segments++;
      if (!aabb_intersect(m, p->o, p->d, &p->is)) {
        float* px = out + 4 * (size_t)p->image_id; /* atomicVectorAdd(T * Le), Le = 1 */
        px[0] += p->T.x;
        px[1] += p->T.y;
        px[2] += p->T.z;
        px[3] = 1.0f;
        st.escaped++;
        p->active = 0;
      } else {
        float sampled = 0.0f;
        int collided = 0;
        uint32_t ns = 0, nd = 0;
        if (p->is.inside) {
          sampled = woodcock(m, p->o, p->d, p->is.dist, &p->rng, &ns, &nd, L->world_to_aabb);
          collided = sampled < p->is.dist;
        }
        st.steps += ns;
        st.density += nd;
        if (!collided) {
          frame_t fr = frame_from_z(p->is.normal);
          f3 dir = frame_to_local(&fr, normalize3(neg3(p->d)));
          p->o = add3(p->o, scl3(p->d, p->is.dist));
          float weight = 1.0f;
          if (ggx_sample(m, dir, &p->rng, &p->d, &weight)) {
            p->T = scl3(p->T, weight);
            p->d = frame_to_world(&fr, p->d);
            p->o = add3(p->o, scl3(p->d, EPS));
          }
        } else {
          p->o = add3(p->o, scl3(p->d, sampled)); /* no -eps (:212) */
          f3 bmin = mk3(m->box_min[0], m->box_min[1], m->box_min[2]);
          f3 bmax = mk3(m->box_max[0], m->box_max[1], m->box_max[2]);
          f3 a = albedo_lookup(m, div3(sub3(p->o, bmin), sub3(bmax, bmin)));
          st.albedo++;
          p->T = mul3(p->T, a);
          float e1 = rng_float(&p->rng);
          float e2 = rng_float(&p->rng);
          p->d = hg_sample(p->d, m->g, e1, e2);
        }
      }
      /* roulette (:220-229): runs whether or not the path escaped */
      float q = det_fminf(1.0f, det_fmaxf(det_fmaxf(p->T.x, p->T.y), p->T.z));
      if (rng_float(&p->rng) > q) p->active = 0;
      p->T = mk3(p->T.x / q, p->T.y / q, p->T.z / q);
    }
  }
  free(th);
  if (stats) *stats = st;
  return 0;
}

/* ------------------------------- thread-bound streamingSK / sortingSK -- */
/* StreamingVolPTsk_kernel::BlockStreamingVolPT::render (StreamingVolPTsk_kernel.cuh
 * :328-349; kSortingRays, the variant d_render defaults to, :373-381) and
 * SortingVolPTsk_kernel::BlockSortingVolPT::render (SortingVolPTsk_kernel.cuh
 * :306-330) with the reference's RNG binding (CVR_OPT_RNG_BINDING 1):
 * one block of n_threads threads (STREAMING_THREADS_BLOCK = 256, Defines.h:21,
 * ITEMS_PER_THREAD 1), thread tid owning Rng(seed + tid) (:341) for whatever
 * path it holds; a path moves between threads at every compaction, its RNG
 * does not.  One iteration of the block:
 *   - regenerate (:66-105): every thread is active; a thread with tid >=
 *     n_active takes a new path unless the head has reached n_paths.  Restated
 *     in lockstep: the head is read once, the requesting threads take
 *     consecutive ids in thread order and the head advances by their number
 *     (so it can pass n_paths, as it does when a warp's atomics race);
 *   - extend: each active thread runs segments (fresh SimpleIsect, scatter at
 *     o + d t - d eps, roulette after every segment, an escape included) until
 *     its path ends or, streamingSK (:284-286), while head > n_paths; sortingSK
 *     (:193-277) decides once per extend, should_regenerate = head <= n_paths:
 *     then it runs one segment per iteration and a collision defers its albedo
 *     (texture_access) past the roulette, otherwise it loops and multiplies
 *     the albedo at once;
 *   - compaction (MortonSort.h:28-49, :188-216): keys = 30-bit Morton code of
 *     the ray origin in the box (AABB::transform, morton3D, Utilities.h:35-55),
 *     morton3D(1,1,1) for inactive threads; a stable sort (cub BlockRadixSort)
 *     gives thread j the path of the thread holding the j-th smallest key;
 *     n_active = the number of active threads; sortingSK then applies each
 *     deferred albedo at the moved path's origin (:118-124).
 * The block loops while n_active > 0 || head < n_paths (:349). */
typedef struct {
  xorwow_t rng;
  f3 o, d, T;
  uint32_t image_id, nseg;
  int active, texacc;
} st_thread_t;

static uint32_t expand_bits10(uint32_t v) { /* Utilities.h:35-41 */
  v = (v * 0x00010001u) & 0xFF0000FFu;
  v = (v * 0x00000101u) & 0x0F00F00Fu;
  v = (v * 0x00000011u) & 0xC30C30C3u;
  v = (v * 0x00000005u) & 0x49249249u;
  return v;
}
static uint32_t morton3d(float x, float y, float z) { /* Utilities.h:45-55 */
  x = det_fminf(det_fmaxf(x * 1024.0f, 0.0f), 1023.0f);
  y = det_fminf(det_fmaxf(y * 1024.0f, 0.0f), 1023.0f);
  z = det_fminf(det_fmaxf(z * 1024.0f, 0.0f), 1023.0f);
  return expand_bits10((uint32_t)x) * 4u + expand_bits10((uint32_t)y) * 2u + expand_bits10((uint32_t)z);
}
static int cmp_u64(const void* a, const void* b) {
  const uint64_t x = *(const uint64_t*)a, y = *(const uint64_t*)b;
  return x < y ? -1 : x > y;
}

EXPORT int oracle_render_stream_thread_bound(const oracle_medium* m, const oracle_launch* L, uint32_t n_threads,
                                             uint32_t first, uint32_t count, int sorting, float* out,
                                             oracle_stats* stats) {
  if (n_threads == 0 || n_threads > 1024) return -1;
  st_thread_t* th = (st_thread_t*)calloc(n_threads, sizeof(st_thread_t));
  st_thread_t* tmp = (st_thread_t*)calloc(n_threads, sizeof(st_thread_t));
  uint64_t* key = (uint64_t*)calloc(n_threads, sizeof(uint64_t));
  if (!th || !tmp || !key) {
    free(th);
    free(tmp);
    free(key);
    return -1;
  }
  oracle_stats st;
  memset(&st, 0, sizeof(st));
  const uint32_t tile_px = (uint32_t)(L->tile_res[0] * L->tile_res[1]);
  const f3 bmin = mk3(m->box_min[0], m->box_min[1], m->box_min[2]);
  const f3 bmax = mk3(m->box_max[0], m->box_max[1], m->box_max[2]);
  const uint32_t code_max = morton3d(1.0f, 1.0f, 1.0f);
  for (uint32_t t = 0; t < n_threads; ++t) rng_init(&th[t].rng, (int32_t)(L->seed_base + t)); /* Q3 */
  uint32_t head = 0, n_active = 0;
  do {
    /* regenerate */
    const uint32_t h0 = head;
    uint32_t req = 0;
    for (uint32_t t = 0; t < n_threads; ++t) {
      st_thread_t* p = &th[t];
      p->active = 1;
      if (t < n_active) continue;
      if (h0 >= count) {
        p->active = 0;
        continue;
      }
      const uint32_t h = h0 + req++;
      if (h >= count) {
        p->active = 0;
        continue;
      }
      const uint32_t path_id = first + h;
      p->image_id = path_id % tile_px;
      float px = (float)(p->image_id % (uint32_t)L->tile_res[0]) + (float)L->offset[0];
      float py = det_floorf((float)p->image_id / L->tile_res[0]) + (float)L->offset[1];
      camera_ray(L, px, py, &p->rng, &p->o, &p->d);
      p->T = mk3(1.0f, 1.0f, 1.0f);
      p->nseg = 0;
      st.paths++;
    }
    if (h0 < count) head = h0 + req;
    /* extend */
    const int should_regenerate = head <= count; /* sortingSK, read once per extend */
    for (uint32_t t = 0; t < n_threads; ++t) {
      st_thread_t* p = &th[t];
      p->texacc = 0;
      if (!p->active) continue;
      do {
        if (L->max_segments && p->nseg >= L->max_segments) { /* safety cap, as the path-bound walk */
          st.truncated++;
          p->active = 0;
          break;
        }
        p->nseg++;
        st.segments++;
        isect_t is;
        is.dist = 0.0f;
        is.normal = mk3(0, 0, 0);
        is.inside = 0;
        if (!aabb_intersect(m, p->o, p->d, &is)) {
          float* px = out + 4 * (size_t)p->image_id; /* atomicVectorAdd(T * Le), Le = 1 */
          px[0] += p->T.x;
          px[1] += p->T.y;
          px[2] += p->T.z;
          px[3] = 1.0f;
          st.escaped++;
          p->active = 0;
        } else {
          float sampled = 0.0f;
          int collided = 0;
          uint32_t ns = 0, nd = 0;
          if (is.inside) {
            sampled = woodcock(m, p->o, p->d, is.dist, &p->rng, &ns, &nd, L->world_to_aabb);
            collided = sampled < is.dist;
          }
          st.steps += ns;
          st.density += nd;
          if (!collided) {
            frame_t fr = frame_from_z(is.normal);
            f3 dir = frame_to_local(&fr, normalize3(neg3(p->d)));
            p->o = add3(p->o, scl3(p->d, is.dist));
            float weight = 1.0f;
            if (ggx_sample(m, dir, &p->rng, &p->d, &weight)) {
              p->T = scl3(p->T, weight);
              p->d = frame_to_world(&fr, p->d);
              p->o = add3(p->o, scl3(p->d, EPS));
            }
          } else {
            p->o = sub3(add3(p->o, scl3(p->d, sampled)), scl3(p->d, EPS));
            st.albedo++;
            if (sorting && should_regenerate) {
              p->texacc = 1; /* delayed texture access (SortingVolPTsk_kernel.cuh:230-237) */
            } else {
              p->T = mul3(p->T, albedo_lookup(m, div3(sub3(p->o, bmin), sub3(bmax, bmin))));
            }
            float e1 = rng_float(&p->rng);
            float e2 = rng_float(&p->rng);
            p->d = hg_sample(p->d, m->g, e1, e2);
          }
        }
        /* roulette: after every segment, an escape included; T / p either way */
        float q = det_fminf(1.0f, det_fmaxf(det_fmaxf(p->T.x, p->T.y), p->T.z));
        if (rng_float(&p->rng) > q) p->active = 0;
        p->T = mk3(p->T.x / q, p->T.y / q, p->T.z / q);
      } while ((sorting ? !should_regenerate : head > count) && p->active);
    }
    /* compaction: stable Morton sort of the threads' paths, RNGs stay */
    n_active = 0;
    for (uint32_t t = 0; t < n_threads; ++t) {
      const st_thread_t* p = &th[t];
      uint32_t code = code_max;
      if (p->active) {
        const f3 c = div3(sub3(p->o, bmin), sub3(bmax, bmin)); /* AABB::transform */
        code = morton3d(c.x, c.y, c.z);
        n_active++;
      }
      key[t] = ((uint64_t)code << 10) | t;
    }
    qsort(key, n_threads, sizeof(uint64_t), cmp_u64);
    memcpy(tmp, th, n_threads * sizeof(st_thread_t));
    for (uint32_t j = 0; j < n_threads; ++j) {
      const st_thread_t* src = &tmp[key[j] & 1023u];
      st_thread_t* dst = &th[j];
      dst->o = src->o;
      dst->d = src->d;
      dst->T = src->T;
      dst->image_id = src->image_id;
      dst->nseg = src->nseg;
      if (sorting && src->texacc) /* the deferred albedo at the moved path's origin */
        dst->T = mul3(dst->T, albedo_lookup(m, div3(sub3(dst->o, bmin), sub3(bmax, bmin))));
    }
  } while (n_active > 0 || head < count);
  free(th);
  free(tmp);
  free(key);
  if (stats) *stats = st;
  return 0;
}

/* ------------------------------------- thread-bound streamingMK ------- */
/* StreamingVolPTmk::launchRender (RenderKernelLauncher.cu:435-470) with its
 * kernels d_regenerate / d_extend (StreamingVolPTmk_kernel.cuh:26-69,
 * :74-253) and their RNG binding (CVR_OPT_RNG_BINDING 1): one block
 * of n_threads threads (STREAMING_THREADS_BLOCK, ITEMS_PER_THREAD 1), slot j
 * = thread j.  Per iteration:
 *   - regenerate: every slot j >= n_active takes a new path (unless the head
 *     has reached n_paths), Rng(seed + path_id) for its camera ray, and that
 *     RNG becomes thread j's state (states[tid] = rng.getState(), :66);
 *     lockstep as in oracle_render_stream_thread_bound: the head is read once
 *     and the requesting slots take consecutive ids in thread order;
 *   - extend: thread j continues from states[j] whatever path slot j holds;
 *     an active path runs a segment (scatter at o + d t - d eps, roulette after
 *     every segment, an escape included, :194, :203-210) and loops while head >= n_paths
 *     (:212-214); thread j's state is stored back (:241);
 *   - compaction: the active paths in thread order (BlockScan, :229-252) go to
 *     slots 0 .. n_active - 1; the states stay with the threads.
 * The launcher loops while n_active > 0 || head < n_paths (:439). */
EXPORT int oracle_render_smk_thread_bound(const oracle_medium* m, const oracle_launch* L, uint32_t n_threads,
                                          uint32_t first, uint32_t count, float* out, oracle_stats* stats) {
  if (n_threads == 0 || n_threads > 1024) return -1;
  st_thread_t* sl = (st_thread_t*)calloc(n_threads, sizeof(st_thread_t)); /* slots: path + active */
  st_thread_t* nx = (st_thread_t*)calloc(n_threads, sizeof(st_thread_t));
  xorwow_t* state = (xorwow_t*)calloc(n_threads, sizeof(xorwow_t));        /* states[tid] */
  if (!sl || !nx || !state) {
    free(sl);
    free(nx);
    free(state);
    return -1;
  }
  oracle_stats st;
  memset(&st, 0, sizeof(st));
  const uint32_t tile_px = (uint32_t)(L->tile_res[0] * L->tile_res[1]);
  const f3 bmin = mk3(m->box_min[0], m->box_min[1], m->box_min[2]);
  const f3 bmax = mk3(m->box_max[0], m->box_max[1], m->box_max[2]);
  uint32_t head = 0, n_active = 0;
  do {
    /* regenerate */
    const uint32_t h0 = head;
    uint32_t req = 0;
    for (uint32_t t = n_active; t < n_threads; ++t) {
      st_thread_t* p = &sl[t];
      p->active = 0;
      if (h0 >= count) continue;
      const uint32_t h = h0 + req++;
      if (h >= count) continue;
      const uint32_t path_id = first + h;
      p->image_id = path_id % tile_px;
      float px = (float)(p->image_id % (uint32_t)L->tile_res[0]) + (float)L->offset[0];
      float py = det_floorf((float)p->image_id / L->tile_res[0]) + (float)L->offset[1];
      xorwow_t rng;
      rng_init(&rng, (int32_t)(L->seed_base + path_id)); /* Rng(c_seed + path_id), Q3 */
      camera_ray(L, px, py, &rng, &p->o, &p->d);
      state[t] = rng;
      p->T = mk3(1.0f, 1.0f, 1.0f);
      p->nseg = 0;
      p->active = 1;
      st.paths++;
    }
    if (h0 < count) head = h0 + req;
    /* extend */
    for (uint32_t t = 0; t < n_threads; ++t) {
      st_thread_t* p = &sl[t];
      xorwow_t* rng = &state[t];
      if (!p->active) continue;
      do {
        if (L->max_segments && p->nseg >= L->max_segments) { /* safety cap, as the path-bound walk */
          st.truncated++;
          p->active = 0;
          break;
        }
        p->nseg++;
        st.segments++;
        isect_t is;
        is.dist = 0.0f;
        is.normal = mk3(0, 0, 0);
        is.inside = 0;
        if (!aabb_intersect(m, p->o, p->d, &is)) {
          float* px = out + 4 * (size_t)p->image_id; /* atomicVectorAdd(T * Le), Le = 1 */
          px[0] += p->T.x;
          px[1] += p->T.y;
          px[2] += p->T.z;
          px[3] = 1.0f;
          st.escaped++;
          p->active = 0;
        } else {
          float sampled = 0.0f;
          int collided = 0;
          uint32_t ns = 0, nd = 0;
          if (is.inside) {
            sampled = woodcock(m, p->o, p->d, is.dist, rng, &ns, &nd, L->world_to_aabb);
            collided = sampled < is.dist;
          }
          st.steps += ns;
          st.density += nd;
          if (!collided) {
            frame_t fr = frame_from_z(is.normal);
            f3 dir = frame_to_local(&fr, normalize3(neg3(p->d)));
            p->o = add3(p->o, scl3(p->d, is.dist));
            float weight = 1.0f;
            if (ggx_sample(m, dir, rng, &p->d, &weight)) {
              p->T = scl3(p->T, weight);
              p->d = frame_to_world(&fr, p->d);
              p->o = add3(p->o, scl3(p->d, EPS));
            }
          } else {
            p->o = sub3(add3(p->o, scl3(p->d, sampled)), scl3(p->d, EPS));
            st.albedo++;
            p->T = mul3(p->T, albedo_lookup(m, div3(sub3(p->o, bmin), sub3(bmax, bmin))));
            float e1 = rng_float(rng);
            float e2 = rng_float(rng);
            p->d = hg_sample(p->d, m->g, e1, e2);
          }
        }
        float q = det_fminf(1.0f, det_fmaxf(det_fmaxf(p->T.x, p->T.y), p->T.z));
        if (rng_float(rng) > q) p->active = 0;
        p->T = mk3(p->T.x / q, p->T.y / q, p->T.z / q);
      } while (head >= count && p->active);
    }
    /* compaction: the active paths in thread order; the states stay */
    n_active = 0;
    for (uint32_t t = 0; t < n_threads; ++t)
      if (sl[t].active) nx[n_active++] = sl[t];
    for (uint32_t t = 0; t < n_active; ++t) sl[t] = nx[t];
  } while (n_active > 0 || head < count);
  free(sl);
  free(nx);
  free(state);
  if (stats) *stats = st;
  return 0;
}

/* ----------------------------------------------------- unit probes ----- */
/* Small entry points used by the known-answer tests. */
EXPORT void oracle_rng_stream(int32_t seed, uint32_t n, uint32_t* out_u32, float* out_f) {
  xorwow_t s;
  rng_init(&s, seed);
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t u = rng_next(&s);
    if (out_u32) out_u32[i] = u;
    if (out_f) out_f[i] = det_fmaf((float)u, 2.3283064e-10f, 1.1641532e-10f);
  }
}
EXPORT void oracle_rng_state(int32_t seed, uint32_t out[6]) {
  xorwow_t s;
  rng_init(&s, seed);
  memcpy(out, s.v, 5 * sizeof(uint32_t));
  out[5] = s.d;
}
/* The seeding structure with other scramble constants (the rocRAND pin). */
EXPORT void oracle_rng_state_consts(unsigned long long seed, uint32_t x0, uint32_t x1, uint32_t m0, uint32_t m1,
                                    uint32_t out[6]) {
  xorwow_t s;
  rng_init_consts(&s, seed, x0, x1, m0, m1);
  memcpy(out, s.v, 5 * sizeof(uint32_t));
  out[5] = s.d;
}
EXPORT float oracle_density(const oracle_medium* m, const float p[3]) {
  return density_lookup(m, mk3(p[0], p[1], p[2]));
}
EXPORT int oracle_aabb(const oracle_medium* m, const float o[3], const float d[3], float out[5]) {
  isect_t is;
  is.dist = 0.0f;
  is.normal = mk3(0, 0, 0);
  is.inside = 0;
  int hit = aabb_intersect(m, mk3(o[0], o[1], o[2]), mk3(d[0], d[1], d[2]), &is);
  out[0] = is.dist;
  out[1] = is.normal.x;
  out[2] = is.normal.y;
  out[3] = is.normal.z;
  out[4] = (float)is.inside;
  return hit;
}
EXPORT void oracle_hg(const float v[3], float g, float e1, float e2, float out[3]) {
  f3 r = hg_sample(mk3(v[0], v[1], v[2]), g, e1, e2);
  out[0] = r.x;
  out[1] = r.y;
  out[2] = r.z;
}
EXPORT float oracle_fresnel(float eta, float ndotwi, float* ndotwt) {
  return fresnel_dielectric(eta, ndotwi, ndotwt);
}
EXPORT float oracle_ggx_g1(float ax, float ay, const float v[3], const float m[3]) {
  return ggx_g1(ax, ay, mk3(v[0], v[1], v[2]), mk3(m[0], m[1], m[2]));
}
EXPORT void oracle_ggx_vndf(const float wi[3], float ax, float ay, float sx, float sy, float out[3]) {
  f3 r = ggx_sample_vndf(mk3(wi[0], wi[1], wi[2]), ax, ay, sx, sy);
  out[0] = r.x;
  out[1] = r.y;
  out[2] = r.z;
}
/* out: wo[3] and the weight.  wo starts as NaN: a failed sample may leave it unwritten (Q8). */
EXPORT int oracle_ggx_sample(const float roughness[2], float eta, const float wi[3], int32_t seed, float out[4]) {
  oracle_medium m;
  memset(&m, 0, sizeof(m));
  m.roughness[0] = roughness[0];
  m.roughness[1] = roughness[1];
  m.eta = eta;
  xorwow_t rng;
  rng_init(&rng, seed);
  const float nan = __builtin_nanf("");
  f3 wo = mk3(nan, nan, nan);
  float weight = nan;
  int ok = ggx_sample(&m, mk3(wi[0], wi[1], wi[2]), &rng, &wo, &weight);
  out[0] = wo.x;
  out[1] = wo.y;
  out[2] = wo.z;
  out[3] = weight;
  return ok;
}
/* out: the frame's x, y and z axes, three floats each */
EXPORT void oracle_frame(const float n[3], float out[9]) {
  frame_t f = frame_from_z(mk3(n[0], n[1], n[2]));
  out[0] = f.x.x; out[1] = f.x.y; out[2] = f.x.z;
  out[3] = f.y.x; out[4] = f.y.y; out[5] = f.y.z;
  out[6] = f.z.x; out[7] = f.z.y; out[8] = f.z.z;
}
EXPORT void oracle_camera_ray(const oracle_launch* L, uint32_t path_id, float out[6]) {
  const uint32_t tile_px = (uint32_t)(L->tile_res[0] * L->tile_res[1]);
  const uint32_t image_id = path_id % tile_px;
  xorwow_t rng;
  rng_init(&rng, (int32_t)(L->seed_base + path_id));
  float px = (float)(image_id % (uint32_t)L->tile_res[0]) + (float)L->offset[0];
  float py = det_floorf((float)image_id / L->tile_res[0]) + (float)L->offset[1];
  f3 o, d;
  camera_ray(L, px, py, &rng, &o, &d);
  out[0] = o.x; out[1] = o.y; out[2] = o.z;
  out[3] = d.x; out[4] = d.y; out[5] = d.z;
}
EXPORT void oracle_detmath(int fn, const float* x, const float* y, uint32_t n, float* out) {
  for (uint32_t i = 0; i < n; ++i) {
    switch (fn) {
      case 0: out[i] = det_logf(x[i]); break;
      case 1: out[i] = det_sinf(x[i]); break;
      case 2: out[i] = det_cosf(x[i]); break;
      case 3: out[i] = det_tanf(x[i]); break;
      case 4: out[i] = det_acosf(x[i]); break;
      case 5: out[i] = det_atan2f(y[i], x[i]); break;
      default: out[i] = 0.0f;
    }
  }
}
