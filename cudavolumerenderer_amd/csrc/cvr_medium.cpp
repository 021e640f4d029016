// cvr_medium.cpp - the medium of a context: the host uploads (dense, sparse) and the build from
// device memory (two arrays, or a scalar field and a 1-D, gradient-magnitude or per-label transfer
// function: build_from_device) through one set of stages, the transfer functions' host statements, and what
// the context tells of the result.
//
// Each rule is stated once: the shape guards (dense_shape_check, sparse_shape_check), the dense
// build from the grids on (finish_dense), the sparse build from a leaf table in device memory on
// (finish_sparse).  The cell-leaf rule and the empty-region mask's bits are cvr_medium_build.hip's.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "cvr_ctx.h"

using cvr::ensure_device;
using cvr::set_err;

namespace cvr {
float half_round1(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  const uint32_t sign = u & 0x80000000u, a = u & 0x7FFFFFFFu;
  uint32_t r;
  if (a >= 0x7F800000u) {
    // inf stays inf; NaN keeps its top 10 payload bits and stays NaN (quiet bit set if they are all 0)
    r = a == 0x7F800000u ? a : ((a & 0xFFFFE000u) | 0x00400000u);
  } else if (a >= 0x477FF000u) {
    r = 0x7F800000u;  // >= 65520: rounds to inf
  } else if (a >= 0x38800000u) {
    // normal half: keep 10 mantissa bits, nearest even on the 13 dropped (a carry moves to the next
    // exponent, at most to 65504's successor, excluded above)
    r = (a + 0x00000FFFu + ((a >> 13) & 1u)) & 0xFFFFE000u;
  } else {
    // below 2^-14: multiples of 2^-24.  Adding 2^-1 (ulp 2^-24 in [0.5, 1)) rounds to nearest even.
    float t;
    memcpy(&t, &a, 4);
    const float k = (t + 0.5f) - 0.5f;
    memcpy(&r, &k, 4);
  }
  r |= sign;
  float o;
  memcpy(&o, &r, 4);
  return o;
}
// f is finite and rounds to +-inf: 65520 <= |f| < inf, one unsigned compare of |f|'s bits
static inline bool overflows_half(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return (u & 0x7FFFFFFFu) - 0x477FF000u < 0x7F800000u - 0x477FF000u;
}
bool half_overflows(const float* v, size_t n, size_t stride, size_t take, size_t* at) {
  // a block of groups at a time without an exit, which the compiler vectorises; a block that
  // holds such a value is then searched in order
  constexpr size_t kBlock = 1024;
  for (size_t i0 = 0; i0 < n; i0 += kBlock) {
    const size_t i1 = std::min(n, i0 + kBlock);
    bool any = false;
    for (size_t i = i0; i < i1; ++i)
      for (size_t k = 0; k < take; ++k) any |= overflows_half(v[i * stride + k]);
    if (!any) continue;
    for (size_t i = i0; i < i1; ++i)
      for (size_t k = 0; k < take; ++k)
        if (overflows_half(v[i * stride + k])) {
          *at = i * stride + k;
          return true;
        }
  }
  return false;
}
float half_majorant(float max_density) {
  const float h = half_round1(max_density);
  return (std::isfinite(h) && h > max_density) ? h : max_density;
}

void free_sparse(cvr_ctx* c) {
  if (c->d_leaves) (void)hipFree(c->d_leaves);
  if (c->d_leaf_density) (void)hipFree(c->d_leaf_density);
  if (c->d_leaf_albedo) (void)hipFree(c->d_leaf_albedo);
  if (c->d_sbounds) (void)hipFree(c->d_sbounds);
  if (c->d_emask) (void)hipFree(c->d_emask);
  c->d_emask = nullptr;
  c->d_leaves = nullptr;
  c->d_leaf_density = nullptr;
  c->d_leaf_albedo = nullptr;
  c->d_sbounds = nullptr;
  c->n_cell_leaves = 0;
}
void drop_dense(cvr_ctx* c) {
  if (c->d_density) (void)hipFree(c->d_density);
  if (c->d_albedo) (void)hipFree(c->d_albedo);
  if (c->d_cells) (void)hipFree(c->d_cells);
  if (c->d_bounds) (void)hipFree(c->d_bounds);
  c->d_density = nullptr;
  c->d_albedo = nullptr;
  c->d_cells = nullptr;
  c->d_bounds = nullptr;
  c->n_voxels = 0;
}
// p is memory the context's device can read, by what the runtime knows of it: device memory of
// that device, managed memory, or mapped host memory (an address HIP does not know is refused)
bool device_readable(const cvr_ctx* c, const void* p) {
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  if (at.type == hipMemoryTypeDevice) return at.device == c->device;
  return (at.type == hipMemoryTypeManaged || at.type == hipMemoryTypeHost) && at.devicePointer != nullptr;
}
}  // namespace cvr

using cvr::drop_dense;
using cvr::free_sparse;
using cvr::half_majorant;
using cvr::half_overflows;
using cvr::half_round1;

namespace {
// Device allocations of one call, freed on every way out of it (keep(): the context owns it now)
struct DevTemps {
  std::vector<void*> p;
  ~DevTemps() {
    for (void* q : p) (void)hipFree(q);
  }
  hipError_t alloc(void** out, size_t bytes) {
    const hipError_t e = hipMalloc(out, bytes ? bytes : 4);
    if (e == hipSuccess) p.push_back(*out);
    return e;
  }
  void keep(void* q) { p.erase(std::remove(p.begin(), p.end(), q), p.end()); }
};
// Device time of the launches between begin() and end(i), added to devmed_ms[i] (CVR_OPT_TIMING;
// without it no event and no synchronisation)
struct DevmedTimer {
  cvr_ctx* c;
  hipEvent_t a = nullptr, b = nullptr;
  bool on;
  explicit DevmedTimer(cvr_ctx* ctx) : c(ctx), on(ctx->wf_timing) {
    for (double& v : c->devmed_ms) v = 0.0;
    if (on) on = hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess;
  }
  ~DevmedTimer() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
  void begin() {
    if (on) (void)hipEventRecord(a, c->stream);
  }
  void end(int i) {
    float ms = 0.f;
    if (on && hipEventRecord(b, c->stream) == hipSuccess && hipEventSynchronize(b) == hipSuccess &&
        hipEventElapsedTime(&ms, a, b) == hipSuccess)
      c->devmed_ms[i] += ms;
  }
};
using cvr::device_readable;
using cvr::overflows_half;

// What the three descriptors say of the medium besides its arrays
struct MediumView {
  const uint32_t* res;
  const float *box_min, *box_max;
  float scale, g;
  const float* roughness;
  float eta;
};
template <class Desc>
MediumView view_of(const Desc& d) {
  return {d.res, d.box_min, d.box_max, d.scale, d.g, d.roughness, d.eta};
}

// Geometry, scale and BSDF parameters shared by the dense and sparse media
// (HeterogeneousMedium + GGX, Medium.h:110-190).
void fill_medium_common(cvr::MediumParams& m, const MediumView& v, float max_density) {
  const uint32_t* res = v.res;
  m.rx = res[0];
  m.ry = res[1];
  m.rz = res[2];
  m.rxy = res[0] * res[1];  // only used by dense media, where it is < 2^24
  m.fres_x = (float)res[0];
  m.fres_y = (float)res[1];
  m.fres_z = (float)res[2];
  m.gx = m.agx = (float)(res[0] - 1u);
  m.gy = m.agy = (float)(res[1] - 1u);
  m.gz = m.agz = (float)(res[2] - 1u);
  m.bmin = cvr::V3{v.box_min[0], v.box_min[1], v.box_min[2]};
  m.bmax = cvr::V3{v.box_max[0], v.box_max[1], v.box_max[2]};
  const float ex = v.box_max[0] - v.box_min[0], ey = v.box_max[1] - v.box_min[1], ez = v.box_max[2] - v.box_min[2];
  m.shift = cvr::V3{v.box_min[0] / ex, v.box_min[1] / ey, v.box_min[2] / ez};
  m.scale = v.scale;
  m.inv_sigma = 1.0f / (v.scale * max_density);
  m.g = v.g;
  m.ax = v.roughness[0];
  m.ay = v.roughness[1];
  m.eta = v.eta;
  m.inv_eta = 1.0f / v.eta;
}

// bytes per density voxel / cell / albedo voxel of a storage format
struct FormatBytes {
  size_t d, c, a;
};
FormatBytes format_bytes(uint32_t fmt) {
  return fmt ? FormatBytes{2, 16, 8} : FormatBytes{sizeof(float), 2 * sizeof(float4), sizeof(float4)};
}
// brick bounds are built (else every brick is unbounded and a sparse medium has no mask)
bool bounded(const cvr_ctx* c, float scale, float max_density) {
  const float sigma = scale * max_density;
  return c->bound_shift && sigma > 0.0f && std::isfinite(sigma) && scale > 0.0f;
}
void set_minfo(cvr_ctx* c, uint32_t fmt, float max_density, size_t density, size_t cells, size_t albedo, size_t bounds) {
  c->minfo = {};
  c->minfo.format = (int32_t)fmt;
  c->minfo.max_density_eff = max_density;
  c->minfo.density_bytes = density;
  c->minfo.cells_bytes = cells;
  c->minfo.albedo_bytes = albedo;
  c->minfo.bounds_bytes = bounds;
  c->minfo.total_bytes = density + cells + albedo + bounds;
}

// ------------------------------------------------------------------- dense ----
// The shape of a dense grid, judged from the numbers alone (before any array is looked at)
int dense_shape_check(cvr_ctx* c, const uint32_t res[3], uint32_t fmt) {
  if (res[0] == 0 || res[1] == 0 || res[2] == 0) return set_err(&c->err, CVR_ERR_INVALID, "empty grid");
  const size_t n = (size_t)res[0] * res[1] * res[2];
  if (n > 0xFFFFFFFFull) return set_err(&c->err, CVR_ERR_INVALID, "grid exceeds 2^32 voxels");
  // the kernels index cells and bricks with 24-bit multiplies
  if ((uint64_t)res[1] * res[2] >= (1ull << 24) || (uint64_t)res[0] * res[1] >= (1ull << 24))
    return set_err(&c->err, CVR_ERR_UNSUPPORTED, "dense grid with y*z or x*y >= 2^24: use cvr_set_medium_sparse");
  // an fp32 cell is two float4: dense_cell doubles the u32 cell index (the half format's cell is one)
  if (!fmt && c->use_cells && n >= (1ull << 31))
    return set_err(&c->err, CVR_ERR_UNSUPPORTED,
                   "dense fp32 grid of %zu voxels (>= 2^31) with density cells: use CVR_OPT_MEDIUM_FORMAT 1, "
                   "CVR_OPT_CELLS 0 or cvr_set_medium_sparse",
                   n);
  return CVR_OK;
}

// The context's density and albedo grids for n voxels of format fmt: the previous dense medium's
// when both match (the grids' bytes depend on the format too), else new ones.  The previous
// medium is gone from here on.
int dense_grids(cvr_ctx* c, size_t n, uint32_t fmt) {
  const FormatBytes B = format_bytes(fmt);
  free_sparse(c);
  c->have_medium = false;
  drop_light_volume(c);
  if (n != c->n_voxels || !c->d_density || c->grids_format != fmt) {
    drop_dense(c);
    HIP_TRY(c, hipMalloc(&c->d_density, n * B.d));
    HIP_TRY(c, hipMalloc(&c->d_albedo, n * B.a));
    c->n_voxels = n;
    c->grids_format = fmt;
  }
  return CVR_OK;
}

// The dense medium from its filled grids on: cells, brick bounds, MediumParams, cvr_medium_info.
// uniform_rgb: null, or the unrounded rgb that every voxel's equals (format 1: after rounding).
int finish_dense(cvr_ctx* c, const MediumView& v, uint32_t fmt, float max_density, const float* uniform_rgb,
                 DevmedTimer& tm) {
  const uint32_t* res = v.res;
  const size_t n = (size_t)res[0] * res[1] * res[2];
  const FormatBytes B = format_bytes(fmt);
  if (c->d_cells) (void)hipFree(c->d_cells);
  c->d_cells = nullptr;
  tm.begin();
  if (c->use_cells) {
    HIP_TRY(c, hipMalloc(&c->d_cells, n * B.c));
    HIP_TRY(c, cvr::launch_build_cells(c->d_density, res[0], res[1], res[2], c->d_cells, c->stream, fmt));
  }
  if (c->d_bounds) (void)hipFree(c->d_bounds);
  c->d_bounds = nullptr;
  size_t bounds_bytes = 0;
  uint32_t bnx = 0, bny = 0, bsentinel = 0;
  if (bounded(c, v.scale, max_density)) {
    const uint32_t S = 1u << c->bound_shift;
    bnx = (res[0] + S - 1) / S;
    bny = (res[1] + S - 1) / S;
    const size_t nb = (size_t)bnx * bny * ((res[2] + S - 1) / S);
    bsentinel = (uint32_t)nb;  // the no-bound entry past the last brick (k_build_bounds writes it)
    HIP_TRY(c, hipMalloc(&c->d_bounds, nb + 1));
    bounds_bytes = nb + 1;
    HIP_TRY(c, cvr::launch_build_bounds(c->d_density, res[0], res[1], res[2], c->bound_shift, max_density,
                                        c->d_bounds, c->stream, fmt));
  }
  tm.end(5);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  cvr::MediumParams& m = c->m;
  m = cvr::MediumParams{};
  m.bounds = c->d_bounds;
  m.bshift = c->bound_shift;
  m.bnx = bnx;
  m.bny = bny;
  m.bnxy = bnx * bny;
  m.bsentinel = bsentinel;
  m.cells = c->d_cells;
  m.density = c->d_density;
  m.albedo = c->d_albedo;
  fill_medium_common(m, v, max_density);
  m.format = fmt;
  if (uniform_rgb) {
    m.albedo_uniform = 1u;
    m.albedo_bg = fmt ? cvr::V3{half_round1(uniform_rgb[0]), half_round1(uniform_rgb[1]), half_round1(uniform_rgb[2])}
                      : cvr::V3{uniform_rgb[0], uniform_rgb[1], uniform_rgb[2]};
  }
  set_minfo(c, fmt, max_density, n * B.d, c->d_cells ? n * B.c : 0, n * B.a, bounds_bytes);
  c->medium_clipped = false;  // (build_from_device notes its clip and its label counts after this)
  c->medium_label_rows = 0;
  memset(c->medium_label_counts, 0, sizeof(c->medium_label_counts));
  c->have_medium = true;
  return CVR_OK;
}

// ------------------------------------------------------------------ sparse ----
// Leaf and brick grids of a sparse medium of resolution res
struct SparseGeom {
  uint32_t ln[3];  // ceil(res / 8)
  size_t nleaf;
  uint32_t bshift, bnx, bny, bnz;
  size_t nb;
};
// The shape of a sparse grid, judged from the numbers alone; fills *g
int sparse_shape_check(cvr_ctx* c, const uint32_t res[3], SparseGeom* g) {
  if (res[0] == 0 || res[1] == 0 || res[2] == 0) return set_err(&c->err, CVR_ERR_INVALID, "empty grid");
  for (int k = 0; k < 3; ++k) g->ln[k] = (res[k] + 7u) / 8u;
  g->nleaf = (size_t)g->ln[0] * g->ln[1] * g->ln[2];
  if (g->nleaf > 0xFFFFFFFFull) return set_err(&c->err, CVR_ERR_INVALID, "leaf table exceeds 2^32 entries");
  // bricks of 2^bshift <= 8 cells (within one leaf); bounds off -> q = 255.
  // Default 8^3 cells per brick: one brick word per leaf's cells (C5: 33.6 MB
  // of words instead of 268 MB at 4^3, so they stay in L2 / Infinity Cache;
  // 12% faster at an unchanged fetch rate, clouds being empty or dense).
  g->bshift = !c->bound_shift_set ? 3u : c->bound_shift == 0 ? 2u : std::min(c->bound_shift, 3u);
  const uint32_t S = 1u << g->bshift;
  g->bnx = (res[0] + S - 1) / S;
  g->bny = (res[1] + S - 1) / S;
  g->bnz = (res[2] + S - 1) / S;
  g->nb = (size_t)g->bnx * g->bny * g->bnz;
  // the kernels index brick words and leaves with 24-bit multiplies, bz * (bnx bny) + by * bnx + bx
  // and (lz * lny + ly) * lnx + lx, and a u32 sum (refused before anything is read or the previous
  // medium is dropped)
  if ((uint64_t)g->bnx * g->bny >= (1ull << 24) || g->bnz > (1u << 24) || g->nb >= 0xFFFFFFFFull)
    return set_err(&c->err, CVR_ERR_UNSUPPORTED,
                   "sparse grid of %ux%ux%u bricks: x*y >= 2^24, z > 2^24 or %zu bricks >= 2^32 - 1 (a larger "
                   "CVR_OPT_BOUNDS brick, up to 8 cells, has fewer)",
                   g->bnx, g->bny, g->bnz, g->nb);
  return CVR_OK;
}

// Empty-region mask (MediumParams::emask): the smallest super-brick of 2^es cells per axis whose
// grid, each axis padded to a power of two (2^lx, 2^ly, ...), fits the 32 kEmaskWords bits.
struct EmaskGeom {
  uint32_t es, lx, ly;
};
EmaskGeom emask_geometry(const uint32_t ln[3]) {
  auto log2up = [](uint32_t v) {
    uint32_t l = 0;
    while ((1u << l) < v) ++l;
    return l;
  };
  uint32_t es = 3, lx = log2up(ln[0]), ly = log2up(ln[1]), lz = log2up(ln[2]);
  while (lx + ly + lz > log2up(32u * cvr::kEmaskWords)) {
    ++es;
    lx -= lx > 0;
    ly -= ly > 0;
    lz -= lz > 0;
  }
  return {es, lx, ly};
}

// What finish_sparse builds from.  d_table is the leaf table (slot or CVR_NO_LEAF per leaf, the
// slots in any order), a DevTemps allocation of g.nleaf words that the context adopts; d_flags
// (g.nleaf words), d_sums (flag_scan_tiles(g.nleaf) words) and d_total (one word) are scratch.
struct SparseBuild {
  MediumView v;
  SparseGeom g;
  uint32_t fmt;
  float max_density;
  const float* bg;   // background albedo, unrounded
  uint32_t n_leaves;  // slots of the pools
  bool albedo_pool;
  uint32_t *d_table, *d_flags, *d_sums, *d_total;
};

// The sparse medium from a leaf table in device memory on.  A leaf's cells read the corners in it
// and its forward neighbours, so it has a cell leaf iff one of those 8 leaves exists; slot 0 is the
// zero leaf.  refuse_overflow() (format 1 only) returns the refusal of values that round to
// infinity, or CVR_OK; it runs after the cell-leaf count's refusal, which keeps the previous
// medium, and leaves the context without one.  fill_pools() fills c->d_leaf_density and, if
// allocated, c->d_leaf_albedo.
template <class Refuse, class Fill>
int finish_sparse(cvr_ctx* c, const SparseBuild& b, DevTemps& tmp, DevmedTimer& tm, Refuse refuse_overflow,
                  Fill fill_pools) {
  const SparseGeom& g = b.g;
  const FormatBytes B = format_bytes(b.fmt);
  hipStream_t s = c->stream;
  tm.begin();
  HIP_TRY(c, cvr::launch_cell_leaf_flags(b.d_table, g.ln, b.d_flags, s));
  HIP_TRY(c, cvr::launch_flag_scan(b.d_flags, g.nleaf, b.d_sums, b.d_total, s));
  tm.end(3);
  HIP_TRY(c, hipStreamSynchronize(s));
  uint32_t total = 0;
  HIP_TRY(c, hipMemcpy(&total, b.d_total, sizeof(total), hipMemcpyDeviceToHost));
  const size_t ncl = (size_t)total + 1;  // slot 0: the zero leaf
  if (ncl > (1u << 24))
    return set_err(&c->err, CVR_ERR_UNSUPPORTED, "sparse medium needs %zu cell leaves (> 2^24)", ncl);
  int r = b.fmt ? refuse_overflow() : CVR_OK;
  if (r) {
    c->have_medium = false;
    drop_light_volume(c);
    return r;
  }
  // drop the previous medium (dense or sparse)
  drop_dense(c);
  c->have_medium = false;
  drop_light_volume(c);
  free_sparse(c);
  tmp.keep(b.d_table);
  c->d_leaves = b.d_table;
  const size_t np = (size_t)b.n_leaves * 512;
  HIP_TRY(c, hipMalloc(&c->d_leaf_density, (np ? np : 1) * B.d));
  if (b.albedo_pool && np) HIP_TRY(c, hipMalloc(&c->d_leaf_albedo, np * B.a));
  tm.begin();
  if ((r = fill_pools())) return r;
  tm.end(4);
  cvr::MediumParams& m = c->m;
  m = cvr::MediumParams{};
  fill_medium_common(m, b.v, b.max_density);
  m.format = b.fmt;
  m.leaves = c->d_leaves;
  m.leaf_density = c->d_leaf_density;
  m.leaf_albedo = c->d_leaf_albedo;
  m.lnx = g.ln[0];
  m.lny = g.ln[1];
  m.albedo_bg = b.fmt ? cvr::V3{half_round1(b.bg[0]), half_round1(b.bg[1]), half_round1(b.bg[2])}
                      : cvr::V3{b.bg[0], b.bg[1], b.bg[2]};
  const int unbounded = !bounded(c, b.v.scale, b.max_density);
  m.bshift = g.bshift;
  m.bnx = g.bnx;
  m.bny = g.bny;
  m.bnxy = g.bnx * g.bny;
  m.bsentinel = (uint32_t)g.nb;  // the no-bound word past the last brick (k_build_sparse_bounds writes it)
  HIP_TRY(c, hipMalloc(&c->d_sbounds, (g.nb + 1) * sizeof(uint32_t)));
  if (c->use_cells) HIP_TRY(c, hipMalloc(&c->d_cells, ncl * 512 * B.c));
  // the mask: bit set iff a leaf of the super-brick has a cell leaf.  Clear super-bricks' brick
  // words are 0 only when bounded.
  const EmaskGeom e = emask_geometry(g.ln);
  if (!unbounded) {
    HIP_TRY(c, hipMalloc(&c->d_emask, cvr::kEmaskWords * sizeof(uint32_t)));
    HIP_TRY(c, hipMemsetAsync(c->d_emask, 0, cvr::kEmaskWords * sizeof(uint32_t), s));
    m.eshift = e.es;
    m.eshy = e.lx;
    m.eshz = e.lx + e.ly;
    m.emask = c->d_emask;
  }
  uint32_t *d_slot = nullptr, *d_coords = nullptr;
  HIP_TRY(c, tmp.alloc((void**)&d_slot, g.nleaf * sizeof(uint32_t)));
  HIP_TRY(c, tmp.alloc((void**)&d_coords, 3 * ncl * sizeof(uint32_t)));
  tm.begin();
  HIP_TRY(c, cvr::launch_scatter_cell_leaves(b.d_flags, g.nleaf, b.d_sums, g.ln, d_slot, d_coords, c->d_emask,
                                             e.es - 3u, e.lx, e.lx + e.ly, s));
  tm.end(3);
  tm.begin();
  HIP_TRY(c, cvr::launch_build_sparse(m, d_coords, c->use_cells ? ncl : 0, d_slot, g.bnz, b.max_density, unbounded,
                                      c->d_cells, c->d_sbounds, s));
  tm.end(5);
  HIP_TRY(c, hipStreamSynchronize(s));
  m.cells = c->d_cells;
  m.sbounds = c->d_sbounds;
  c->n_cell_leaves = ncl;
  set_minfo(c, b.fmt, b.max_density, (np ? np : 1) * B.d, c->d_cells ? ncl * 512 * B.c : 0,
            c->d_leaf_albedo ? np * B.a : 0,
            (g.nb + 1 + g.nleaf + (c->d_emask ? cvr::kEmaskWords : 0)) * sizeof(uint32_t));
  c->medium_clipped = false;  // (build_from_device notes its clip and its label counts after this)
  c->medium_label_rows = 0;
  memset(c->medium_label_counts, 0, sizeof(c->medium_label_counts));
  c->have_medium = true;
  return CVR_OK;
}

// The scratch of finish_sparse's scan, but for the total's word
int alloc_flag_scan(cvr_ctx* c, DevTemps& tmp, SparseBuild* b) {
  HIP_TRY(c, tmp.alloc((void**)&b->d_flags, b->g.nleaf * sizeof(uint32_t)));
  HIP_TRY(c, tmp.alloc((void**)&b->d_sums, cvr::flag_scan_tiles(b->g.nleaf) * sizeof(uint32_t)));
  HIP_TRY(c, tmp.alloc((void**)&b->d_table, b->g.nleaf * sizeof(uint32_t)));
  return CVR_OK;
}

// One voxel's values as a source gives them, for the refusals' messages and the background:
// out = (albedo r, g, b, w, density).  The arrays' source reads them; a classified source reads
// the scalar and classifies it here, which gives the bits the kernels compute.
int source_voxel(cvr_ctx* c, const cvr::VoxelSource& src, const float* host_table, size_t i, bool with_albedo,
                 float out[5]) {
  if (!src.scalar) {
    HIP_TRY(c, hipMemcpy(&out[4], src.density + i, sizeof(float), hipMemcpyDeviceToHost));
    if (with_albedo) HIP_TRY(c, hipMemcpy(out, src.albedo + 4 * i, 4 * sizeof(float), hipMemcpyDeviceToHost));
    return CVR_OK;
  }
  const size_t size = src.scalar_type == CVR_SCALAR_U8 ? 1 : src.scalar_type == CVR_SCALAR_F32 ? 4 : 2;
  alignas(4) unsigned char raw[4];
  // one scalar from the device; the first failure is kept in `failed`, and nothing is copied after it
  // (the 0 a failed read returns reaches no result: `failed` is returned before anything is classified)
  int failed = CVR_OK;
  auto copy = [&](size_t at) -> int {
    HIP_TRY(c, hipMemcpy(raw, static_cast<const unsigned char*>(src.scalar) + at * size, size, hipMemcpyDeviceToHost));
    return CVR_OK;
  };
  auto read = [&](size_t at) {
    if (failed || (failed = copy(at))) return 0.0f;
    return cvr::scalar_voxel(raw, src.scalar_type, 0);
  };
  const float s = read(i);
  float4 e;
  if (src.labels) {
    uint8_t label = 0;
    if (failed) return failed;
    HIP_TRY(c, hipMemcpy(&label, src.labels + i, 1, hipMemcpyDeviceToHost));
    e = cvr::label_classify(s, label, reinterpret_cast<const float4*>(host_table), src.label_rows, src.tf);
  } else if (src.gradient) {
    // the voxel and its up to six in-grid neighbours, as the kernels' stencil reads them
    const uint32_t nx = src.res[0], ny = src.res[1];
    const float mag = cvr::gradient_at(read, (uint32_t)(i % nx), (uint32_t)((i / nx) % ny),
                                       (uint32_t)(i / ((size_t)nx * ny)), src.res, src.gtf.axes);
    if (failed) return failed;
    e = cvr::gradient_classify(s, mag, reinterpret_cast<const float4*>(host_table), src.gtf);
  } else {
    if (failed) return failed;
    e = cvr::transfer_classify(s, reinterpret_cast<const float4*>(host_table), src.tf);
  }
  out[0] = e.x, out[1] = e.y, out[2] = e.z, out[3] = 1.0f, out[4] = e.w;
  return CVR_OK;
}

// The same of a voxel as a build stores it: behind a clip, a voxel the region does not keep is
// (first's albedo, 0), first being the unclipped voxel 0's values.
int stored_voxel(cvr_ctx* c, const cvr::VoxelSource& src, const float* host_table, size_t i, bool with_albedo,
                 const float first[5], float out[5]) {
  if (src.clip) {
    const uint32_t nx = src.res[0], ny = src.res[1];
    if (!cvr::clip_keeps(*src.clip, (uint32_t)(i % nx), (uint32_t)((i / nx) % ny), (uint32_t)(i / ((size_t)nx * ny)))) {
      memcpy(out, first, 4 * sizeof(float));
      out[4] = 0.0f;
      return CVR_OK;
    }
  }
  return source_voxel(c, src, host_table, i, with_albedo, out);
}

// What the descriptors of the two device calls say besides the source
struct DeviceBuild {
  MediumView v;
  uint32_t flags;            // CVR_DEVMED_*
  const float* const_albedo;  // with CVR_DEVMED_CONST_ALBEDO
  float max_density;          // without CVR_DEVMED_MAX_DENSITY
  const float* host_table;    // a classified source's table, in host memory
};
float majorant_of(const DeviceBuild& d, const cvr::MedScan& scan, uint32_t fmt) {
  float max_density = d.max_density;
  if (d.flags & CVR_DEVMED_MAX_DENSITY) memcpy(&max_density, &scan.max_bits, sizeof(float));
  return fmt ? half_majorant(max_density) : max_density;
}

// The sparse half of the device calls: the leaf rule on the device, then finish_sparse.
// `bg`: voxel 0's albedo, or the constant.  scan: the value scans' results (a classified source:
// not yet run; the leaf flags' pass finds them).
int devmed_sparse(cvr_ctx* c, const DeviceBuild& d, const cvr::VoxelSource& src, SparseBuild& b, cvr::MedScan scan,
                  const float bg[4], cvr::MedScan* d_scan, DevTemps& tmp, DevmedTimer& tm) {
  const uint32_t *res = d.v.res, *ln = b.g.ln;
  const size_t nleaf = b.g.nleaf;
  const uint32_t fmt = b.fmt;
  const bool classified = src.scalar != nullptr, konst = (d.flags & CVR_DEVMED_CONST_ALBEDO) != 0;
  // the leaf albedo pool is kept iff some voxel's 16 bytes differ from the background; if none
  // does, no leaf exists through its albedo either and the albedo is not read again
  b.albedo_pool = !konst && (scan.albedo_flags & 2u);
  hipStream_t s = c->stream;
  int r = alloc_flag_scan(c, tmp, &b);
  if (r) return r;
  b.d_total = &d_scan->total[1];
  b.bg = bg;
  // leaves: flags -> scan -> table and slots
  tm.begin();
  HIP_TRY(c, cvr::launch_leaf_flags(src, classified || b.albedo_pool, res, ln, b.d_flags, fmt, d_scan, s));
  tm.end(2);
  tm.begin();
  HIP_TRY(c, cvr::launch_flag_scan(b.d_flags, nleaf, b.d_sums, &d_scan->total[0], s));
  tm.end(3);
  HIP_TRY(c, hipStreamSynchronize(s));
  if (classified) {
    HIP_TRY(c, hipMemcpy(&scan, d_scan, sizeof(scan), hipMemcpyDeviceToHost));
    b.albedo_pool = (scan.albedo_flags & 2u) != 0;
    b.max_density = majorant_of(d, scan, fmt);
    b.n_leaves = scan.total[0];
  } else {
    HIP_TRY(c, hipMemcpy(&b.n_leaves, &d_scan->total[0], sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  const bool with_albedo = b.albedo_pool;
  const uint32_t n_leaves = b.n_leaves;
  uint32_t* d_slot_leaf = nullptr;
  HIP_TRY(c, tmp.alloc((void**)&d_slot_leaf, (size_t)n_leaves * sizeof(uint32_t)));
  tm.begin();
  HIP_TRY(c, cvr::launch_scatter_leaves(b.d_flags, nleaf, b.d_sums, b.d_table, d_slot_leaf, s));
  tm.end(3);
  auto refuse_overflow = [&]() -> int {
    // the host call names the pools' first overflowing index: when the scans of the grid saw an
    // overflow, the gather runs once without storing to find that index
    size_t at = 0;
    const char* what = nullptr;
    float value = 0.0f;
    if (scan.ovf_density != ~0ull || scan.ovf_albedo != ~0ull) {
      cvr::MedScan chk = scan;
      chk.ovf_density = chk.ovf_albedo = ~0ull;
      HIP_TRY(c, hipMemcpy(d_scan, &chk, sizeof(chk), hipMemcpyHostToDevice));
      HIP_TRY(c, cvr::launch_gather_leaves(src, with_albedo, res, ln, d_slot_leaf, n_leaves, bg, fmt, nullptr, nullptr,
                                           d_scan, s));
      HIP_TRY(c, hipStreamSynchronize(s));
      HIP_TRY(c, hipMemcpy(&chk, d_scan, sizeof(chk), hipMemcpyDeviceToHost));
      const bool in_density = chk.ovf_density != ~0ull;
      if (in_density || chk.ovf_albedo != ~0ull) {
        what = in_density ? "leaf density" : "leaf albedo";
        at = (size_t)(in_density ? chk.ovf_density : chk.ovf_albedo);
        // the value, for the message: the pool voxel's grid voxel, or the background's channel
        const size_t p = in_density ? at : at / 4;
        uint32_t leaf = 0;
        HIP_TRY(c, hipMemcpy(&leaf, d_slot_leaf + (p >> 9), sizeof(leaf), hipMemcpyDeviceToHost));
        const uint32_t local = (uint32_t)(p & 511u);
        const uint32_t x = (leaf % ln[0]) * 8u + (local & 7u), y = ((leaf / ln[0]) % ln[1]) * 8u + ((local >> 3) & 7u),
                       z = (leaf / (ln[0] * ln[1])) * 8u + (local >> 6);
        const size_t i = ((size_t)z * res[1] + y) * res[0] + x;
        if (x < res[0] && y < res[1] && z < res[2]) {
          float v[5];
          if ((r = stored_voxel(c, src, d.host_table, i, !in_density, bg, v))) return r;
          value = in_density ? v[4] : v[at % 4];
        } else {
          value = in_density ? 0.0f : bg[at % 4];
        }
      }
    }
    for (size_t k = 0; k < 3 && !what; ++k)
      if (overflows_half(bg[k])) what = "albedo_background", at = k, value = bg[k];
    if (!what) return CVR_OK;
    return set_err(&c->err, CVR_ERR_INVALID, "medium format half: %s value %g at index %zu rounds to infinity", what,
                   (double)value, at);
  };
  auto gather = [&]() -> int {
    HIP_TRY(c, cvr::launch_gather_leaves(src, with_albedo && c->d_leaf_albedo, res, ln, d_slot_leaf, n_leaves, bg, fmt,
                                         c->d_leaf_density, c->d_leaf_albedo, nullptr, s));
    return CVR_OK;
  };
  return finish_sparse(c, b, tmp, tm, refuse_overflow, gather);
}

// n outside 2..4096, unknown flags, a NULL table, lo / hi not finite or hi <= lo, in cvr.h's order
// for cvr_set_medium_scalar (which looks at d_scalar between the table and lo / hi: after_table)
template <class F>
int transfer_check(std::string* err, const cvr_transfer_desc* t, F after_table) {
  if (t->flags & ~(uint32_t)(CVR_TF_CEIL | CVR_TF_DENSITY_U))
    return set_err(err, CVR_ERR_INVALID, "unknown cvr_transfer_desc flags 0x%x", t->flags);
  if (t->n < 2u || t->n > 4096u)
    return set_err(err, CVR_ERR_INVALID, "transfer table of %u entries (2..4096)", t->n);
  if (!t->table) return set_err(err, CVR_ERR_INVALID, "transfer table is NULL");
  if (int r = after_table()) return r;
  if (!std::isfinite(t->lo) || !std::isfinite(t->hi) || !(t->hi > t->lo))
    return set_err(err, CVR_ERR_INVALID, "transfer range lo %g, hi %g: both finite and hi > lo", (double)t->lo,
                   (double)t->hi);
  return CVR_OK;
}

// The 2-D descriptor's refusals in cvr.h's order for cvr_set_medium_gradient (which looks at
// d_scalar with the table: after_table); the spacing's reciprocals go to *p
template <class F>
int gradient_check(std::string* err, const cvr_gradient_transfer_desc* t, F after_table, cvr::GradientParams* p) {
  if (t->n < 2u || t->m < 2u || (uint64_t)t->n * t->m > 4096u)
    return set_err(err, CVR_ERR_INVALID, "gradient transfer table of %u x %u entries (n >= 2, m >= 2, n * m <= 4096)",
                   t->n, t->m);
  if (t->flags || t->reserved)
    return set_err(err, CVR_ERR_INVALID, "cvr_gradient_transfer_desc flags 0x%x, reserved 0x%x: both must be 0",
                   t->flags, t->reserved);
  if (!t->table) return set_err(err, CVR_ERR_INVALID, "transfer table is NULL");
  if (int r = after_table()) return r;
  if (!std::isfinite(t->lo) || !std::isfinite(t->hi) || !(t->hi > t->lo))
    return set_err(err, CVR_ERR_INVALID, "transfer range lo %g, hi %g: both finite and hi > lo", (double)t->lo,
                   (double)t->hi);
  if (!std::isfinite(t->glo) || !std::isfinite(t->ghi) || !(t->glo >= 0.0f) || !(t->ghi > t->glo))
    return set_err(err, CVR_ERR_INVALID, "gradient range glo %g, ghi %g: both finite, glo >= 0 and ghi > glo",
                   (double)t->glo, (double)t->ghi);
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(t->spacing[k]) || !(t->spacing[k] > 0.0f))
      return set_err(err, CVR_ERR_INVALID, "voxel spacing[%d] = %g: finite and > 0", k, (double)t->spacing[k]);
  *p = cvr::GradientParams{t->n, t->m, t->lo, t->hi, t->glo, t->ghi, cvr::gradient_axes(t->spacing)};
  return CVR_OK;
}

// The labelled descriptor's refusals in cvr.h's order for cvr_set_medium_labeled (which looks at
// d_scalar and d_labels with the table: after_table)
template <class F>
int label_transfer_check(std::string* err, const cvr_label_transfer_desc* t, F after_table) {
  if (t->n < 2u || t->m < 1u || t->m > 256u || (uint64_t)t->n * t->m > 4096u)
    return set_err(err, CVR_ERR_INVALID, "label transfer table of %u x %u entries (n >= 2, 1 <= m <= 256, n * m <= 4096)",
                   t->n, t->m);
  if ((t->flags & ~(uint32_t)(CVR_TF_CEIL | CVR_TF_DENSITY_U)) || t->reserved)
    return set_err(err, CVR_ERR_INVALID, "cvr_label_transfer_desc flags 0x%x unknown or reserved 0x%x not 0", t->flags,
                   t->reserved);
  if (!t->table) return set_err(err, CVR_ERR_INVALID, "transfer table is NULL");
  if (int r = after_table()) return r;
  if (!std::isfinite(t->lo) || !std::isfinite(t->hi) || !(t->hi > t->lo))
    return set_err(err, CVR_ERR_INVALID, "transfer range lo %g, hi %g: both finite and hi > lo", (double)t->lo,
                   (double)t->hi);
  return CVR_OK;
}

// Both device calls from their checked arguments on: one sequence of stages for either source.
// b.g is filled for a sparse build; tmp may already hold the call's allocations (the table).
// The context's clip, when set, is taken here: the source then carries the region, every launch
// that takes the source runs its clipped instance, and the medium notes what it was built under.
int build_from_device(cvr_ctx* c, const DeviceBuild& d, const cvr::VoxelSource& unclipped, SparseBuild& b,
                      DevTemps& tmp) {
  const uint32_t* res = d.v.res;
  cvr::VoxelSource src = unclipped;
  cvr::ClipRegion region{};
  const cvr_clip_desc clip = c->clip;
  if (c->clip_set) {
    for (int a = 0; a < 3; ++a) {
      region.lo[a] = clip.lo[a];
      region.hi[a] = std::min(clip.hi[a], res[a]);
    }
    region.n_planes = clip.n_planes;
    memcpy(region.planes, clip.planes, sizeof(region.planes));
    src.clip = &region;
    memcpy(src.res, res, sizeof(src.res));
  }
  const bool sparse = (d.flags & CVR_DEVMED_SPARSE) != 0, konst = (d.flags & CVR_DEVMED_CONST_ALBEDO) != 0;
  const bool classified = src.scalar != nullptr;
  const uint32_t fmt = (uint32_t)c->medium_format;
  const size_t n = (size_t)res[0] * res[1] * res[2];
  int r;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  DevmedTimer tm(c);
  // the value scans: majorant, binary16 overflow, albedo sameness
  cvr::MedScan scan{~0ull, ~0ull, 0u, 0u, {0u, 0u}, {}};
  // the clip the medium was built under and the kept voxels its store or leaf-flag pass counted
  uint32_t* d_label_counts = nullptr;
  auto note_clip = [&](int result, const cvr::MedScan* d_counted) -> int {
    if (result) return result;
    if (src.labels) {
      // the kept voxels per label byte, of the store or leaf-flag pass: the slots' sums
      std::vector<uint32_t> slots((size_t)cvr::kLabelSlots * 256);
      HIP_TRY(c, hipMemcpy(slots.data(), d_label_counts, slots.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
      for (size_t k = 0; k < slots.size(); ++k) c->medium_label_counts[k & 255u] += slots[k];
      c->medium_label_rows = src.label_rows;
    }
    if (!src.clip) return CVR_OK;
    unsigned long long slots[cvr::kKeptSlots], kept = 0;
    HIP_TRY(c, hipMemcpy(slots, d_counted->kept, sizeof(slots), hipMemcpyDeviceToHost));
    for (unsigned long long v : slots) kept += v;
    c->medium_clipped = true;
    c->medium_clip = clip;
    c->medium_kept = kept;
    return CVR_OK;
  };
  cvr::MedScan* d_scan = nullptr;
  HIP_TRY(c, tmp.alloc((void**)&d_scan, sizeof(scan)));
  HIP_TRY(c, hipMemcpy(d_scan, &scan, sizeof(scan), hipMemcpyHostToDevice));
  if (src.labels) {
    HIP_TRY(c, tmp.alloc((void**)&d_label_counts, (size_t)cvr::kLabelSlots * 256 * sizeof(uint32_t)));
    HIP_TRY(c, hipMemsetAsync(d_label_counts, 0, (size_t)cvr::kLabelSlots * 256 * sizeof(uint32_t), c->stream));
    src.label_counts = d_label_counts;
  }
  float first[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (konst) memcpy(first, d.const_albedo, 4 * sizeof(float));
  // voxel 0's values (the background, and what a clipped voxel's albedo is), of the unclipped source
  if (!konst && (r = source_voxel(c, unclipped, d.host_table, 0, true, first))) return r;
  if (src.clip) memcpy(src.clip_a0, first, sizeof(src.clip_a0));
  const bool scan_density = fmt || (d.flags & CVR_DEVMED_MAX_DENSITY),
             scan_albedo = !konst && (fmt || sparse || c->uniform_albedo);
  if (classified) {
    // one pass finds both scans' results; a sparse build finds them in its leaf flags' pass
    if (!sparse && (scan_density || scan_albedo)) {
      tm.begin();
      HIP_TRY(c, cvr::launch_scan_classified(src, n, fmt, d_scan, c->stream));
      tm.end(0);
    }
  } else if (src.clip) {
    // one pass finds both scans' results of the clipped values
    if (scan_density || scan_albedo) {
      cvr::VoxelSource sv = src;
      if (!scan_albedo) sv.albedo = nullptr;
      tm.begin();
      HIP_TRY(c, cvr::launch_scan_clipped(sv, res, fmt, d_scan, c->stream));
      tm.end(0);
    }
  } else {
    if (scan_density) {
      tm.begin();
      HIP_TRY(c, cvr::launch_scan_density(src.density, n, fmt, d_scan, c->stream));
      tm.end(0);
    }
    if (scan_albedo) {
      tm.begin();
      HIP_TRY(c, cvr::launch_scan_albedo(src.albedo, n, fmt, d_scan, c->stream));
      tm.end(1);
    }
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(&scan, d_scan, sizeof(scan), hipMemcpyDeviceToHost));
  const float max_density = majorant_of(d, scan, fmt);
  if (sparse) {
    b.v = d.v;
    b.fmt = fmt;
    b.max_density = max_density;
    return note_clip(devmed_sparse(c, d, src, b, scan, first, d_scan, tmp, tm), d_scan);
  }
  if (fmt) {
    // cvr_set_medium's refusal: density before albedo, the smallest index (a constant albedo's
    // grid overflows first at voxel 0)
    const bool bad_d = scan.ovf_density != ~0ull;
    size_t at = (size_t)scan.ovf_density;
    float value = 0.0f;
    bool bad_a = false;
    float v[5];
    if (bad_d) {
      if ((r = stored_voxel(c, src, d.host_table, at, false, first, v))) return r;
      value = v[4];
    } else if (konst) {
      for (size_t k = 0; k < 3 && !bad_a; ++k)
        if (overflows_half(first[k])) bad_a = true, at = k, value = first[k];
    } else if (scan.ovf_albedo != ~0ull) {
      bad_a = true;
      at = (size_t)scan.ovf_albedo;
      if ((r = stored_voxel(c, src, d.host_table, at / 4, true, first, v))) return r;
      value = v[at % 4];
    }
    if (bad_d || bad_a) {
      c->have_medium = false;
      drop_light_volume(c);
      return set_err(&c->err, CVR_ERR_INVALID, "medium format half: %s value %g at index %zu rounds to infinity",
                     bad_d ? "density" : "albedo", (double)value, at);
    }
  }
  // the grids copied (format 1: converted, straight from the caller's fp32 arrays), classified or filled
  if ((r = dense_grids(c, n, fmt))) return r;
  tm.begin();
  if (classified) {
    HIP_TRY(c, cvr::launch_store_classified(src, n, fmt, c->d_density, c->d_albedo, d_scan, c->stream));
  } else if (src.clip) {
    HIP_TRY(c, cvr::launch_store_clipped(src, res, fmt, c->d_density, konst ? nullptr : c->d_albedo, d_scan, c->stream));
  } else if (fmt) {
    HIP_TRY(c, cvr::launch_to_half(src.density, c->d_density, n, c->stream));
    if (!konst) HIP_TRY(c, cvr::launch_to_half(src.albedo, c->d_albedo, 4 * n, c->stream));
  } else {
    HIP_TRY(c, hipMemcpyAsync(c->d_density, src.density, n * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    if (!konst)
      HIP_TRY(c, hipMemcpyAsync(c->d_albedo, src.albedo, n * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
  }
  if (konst) HIP_TRY(c, cvr::launch_fill_albedo(c->d_albedo, n, fmt, d.const_albedo, c->stream));
  tm.end(4);
  const bool same = c->uniform_albedo && (konst || !(scan.albedo_flags & 1u));
  return note_clip(finish_dense(c, d.v, fmt, max_density, same ? first : nullptr, tm), d_scan);
}

// cvr_set_clip's refusals, in cvr.h's order
int clip_check(std::string* err, const cvr_clip_desc* d) {
  if (!d) return set_err(err, CVR_ERR_INVALID, "cvr_clip_desc is NULL");
  if (d->flags) return set_err(err, CVR_ERR_INVALID, "cvr_clip_desc flags 0x%x: must be 0", d->flags);
  if (d->n_planes > CVR_CLIP_MAX_PLANES)
    return set_err(err, CVR_ERR_INVALID, "%u clip planes (at most %d)", d->n_planes, CVR_CLIP_MAX_PLANES);
  for (int a = 0; a < 3; ++a)
    if (d->lo[a] > d->hi[a])
      return set_err(err, CVR_ERR_INVALID, "crop lo[%d] = %u above hi[%d] = %u", a, d->lo[a], a, d->hi[a]);
  for (uint32_t k = 0; k < d->n_planes; ++k)
    for (int j = 0; j < 4; ++j)
      if (!std::isfinite(d->planes[k][j]))
        return set_err(err, CVR_ERR_INVALID, "clip plane %u coefficient %d = %g: not finite", k, j,
                       (double)d->planes[k][j]);
  for (uint32_t k = 0; k < d->n_planes; ++k)
    if (d->planes[k][0] == 0.0f && d->planes[k][1] == 0.0f && d->planes[k][2] == 0.0f)
      return set_err(err, CVR_ERR_INVALID, "clip plane %u has a zero normal (A = B = C = 0)", k);
  return CVR_OK;
}
// the descriptor that keeps everything
cvr_clip_desc clip_everything() {
  cvr_clip_desc d{};
  d.hi[0] = d.hi[1] = d.hi[2] = 0xFFFFFFFFu;
  return d;
}
}  // namespace

extern "C" {

int cvr_set_medium(cvr_ctx* c, const cvr_medium_desc* md) {
  if (!c || !md) return set_err(c ? &c->err : nullptr, CVR_ERR_INVALID, "NULL argument");
  CVR_NOT_IN_SESSION(c, "cvr_set_medium");
  if (c->clip_set)
    return set_err(&c->err, CVR_ERR_UNSUPPORTED, "cvr_set_medium with a clip set: only the device builds clip (cvr_clear_clip first)");
  // (the shape is judged first, from the numbers alone, then the arrays)
  const uint32_t fmt = (uint32_t)c->medium_format;
  int r = dense_shape_check(c, md->res, fmt);
  if (r) return r;
  const size_t n = (size_t)md->res[0] * md->res[1] * md->res[2];
  if (!md->density || !md->albedo) return set_err(&c->err, CVR_ERR_INVALID, "density/albedo is NULL");
  if (fmt) {
    size_t at = 0;
    const bool bad_d = half_overflows(md->density, n, 1, 1, &at);
    const bool bad_a = !bad_d && half_overflows(md->albedo, n, 4, 3, &at);
    if (bad_d || bad_a) {
      c->have_medium = false;
      drop_light_volume(c);
      return set_err(&c->err, CVR_ERR_INVALID, "medium format half: %s value %g at index %zu rounds to infinity",
                     bad_d ? "density" : "albedo", (double)(bad_d ? md->density : md->albedo)[at], at);
    }
  }
  const float max_density = fmt ? half_majorant(md->max_density) : md->max_density;
  if ((r = ensure_device(c))) return r;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  DevmedTimer tm(c);
  if ((r = dense_grids(c, n, fmt))) return r;
  if (fmt) {
    // fp32 staging -> rounded half grids (converted on the device); the staging is freed before
    // the cells and bounds are built, and in any case before this call returns
    float* stage = nullptr;
    HIP_TRY(c, hipMalloc(&stage, n * sizeof(float4)));
    hipError_t e = hipMemcpy(stage, md->density, n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = cvr::launch_to_half(stage, c->d_density, n, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(stage, md->albedo, n * sizeof(float4), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = cvr::launch_to_half(stage, c->d_albedo, 4 * n, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(stage);
    if (e != hipSuccess) return set_err(&c->err, CVR_ERR_HIP, "half medium upload: %s", hipGetErrorString(e));
  } else {
    HIP_TRY(c, hipMemcpy(c->d_density, md->density, n * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->d_albedo, md->albedo, n * sizeof(float4), hipMemcpyHostToDevice));
  }
  bool same = c->uniform_albedo;
  if (same) {
    // every voxel's rgb bit-identical to the first (the XML smoke scene's constant albedo);
    // format 1: the rounded rgb (voxels that differ may round to the same halves)
    float first[3] = {md->albedo[0], md->albedo[1], md->albedo[2]};
    if (fmt)
      for (float& v : first) v = half_round1(v);
    for (size_t i = 1; i < n && same; ++i) {
      same = memcmp(md->albedo + 4 * i, md->albedo, 3 * sizeof(float)) == 0;
      if (!same && fmt) {
        float v[3];
        for (int k = 0; k < 3; ++k) v[k] = half_round1(md->albedo[4 * i + k]);
        same = memcmp(v, first, sizeof(v)) == 0;
      }
    }
  }
  return finish_dense(c, view_of(*md), fmt, max_density, same ? md->albedo : nullptr, tm);
}

int cvr_set_medium_sparse(cvr_ctx* c, const cvr_sparse_medium_desc* sd) {
  if (!c || !sd) return set_err(c ? &c->err : nullptr, CVR_ERR_INVALID, "NULL argument");
  CVR_NOT_IN_SESSION(c, "cvr_set_medium_sparse");
  if (c->clip_set)
    return set_err(&c->err, CVR_ERR_UNSUPPORTED,
                   "cvr_set_medium_sparse with a clip set: only the device builds clip (cvr_clear_clip first)");
  // (as in cvr_set_medium, the shape is judged first, from the numbers alone, then the arrays;
  // an empty grid is sparse_shape_check's to refuse, before leaf_dims)
  const uint32_t* res = sd->res;
  for (int k = 0; k < 3 && res[0] && res[1] && res[2]; ++k)
    if (sd->leaf_dims[k] != (res[k] + 7u) / 8u)
      return set_err(&c->err, CVR_ERR_INVALID, "leaf_dims[%d] = %u, expected ceil(res/8) = %u", k, sd->leaf_dims[k],
                     (res[k] + 7u) / 8u);
  SparseBuild b{};
  int r = sparse_shape_check(c, res, &b.g);
  if (r) return r;
  const size_t nleaf = b.g.nleaf;
  if (!sd->leaf_table || (sd->n_leaves && !sd->leaf_density))
    return set_err(&c->err, CVR_ERR_INVALID, "leaf table / density pool is NULL");
  for (size_t i = 0; i < nleaf; ++i) {
    const uint32_t v = sd->leaf_table[i];
    if (v != CVR_NO_LEAF && v >= sd->n_leaves)
      return set_err(&c->err, CVR_ERR_INVALID, "leaf table entry %u >= n_leaves %u", v, sd->n_leaves);
  }
  const uint32_t fmt = (uint32_t)c->medium_format;
  const size_t np = (size_t)sd->n_leaves * 512;
  b.v = view_of(*sd);
  b.fmt = fmt;
  b.max_density = fmt ? half_majorant(sd->max_density) : sd->max_density;
  b.bg = sd->albedo_background;
  b.n_leaves = sd->n_leaves;
  b.albedo_pool = sd->leaf_albedo != nullptr;
  if ((r = ensure_device(c))) return r;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  // the table goes to the device, where the cell leaves are counted, before the values are judged
  DevTemps tmp;
  DevmedTimer tm(c);
  if ((r = alloc_flag_scan(c, tmp, &b))) return r;
  HIP_TRY(c, tmp.alloc((void**)&b.d_total, sizeof(uint32_t)));
  HIP_TRY(c, hipMemcpy(b.d_table, sd->leaf_table, nleaf * sizeof(uint32_t), hipMemcpyHostToDevice));
  auto refuse_overflow = [&]() -> int {
    size_t at = 0;
    const char* what = nullptr;
    const float* arr = nullptr;
    if (half_overflows(sd->leaf_density, np, 1, 1, &at)) what = "leaf density", arr = sd->leaf_density;
    else if (sd->leaf_albedo && half_overflows(sd->leaf_albedo, np, 4, 3, &at)) what = "leaf albedo", arr = sd->leaf_albedo;
    else if (half_overflows(sd->albedo_background, 1, 4, 3, &at)) what = "albedo_background", arr = sd->albedo_background;
    if (!what) return CVR_OK;
    return set_err(&c->err, CVR_ERR_INVALID, "medium format half: %s value %g at index %zu rounds to infinity", what,
                   (double)arr[at], at);
  };
  auto upload = [&]() -> int {
    if (fmt && np) {
      // fp32 staging -> rounded half pools (converted on the device), freed before the cells are built
      float* stage = nullptr;
      HIP_TRY(c, hipMalloc(&stage, np * (c->d_leaf_albedo ? sizeof(float4) : sizeof(float))));
      hipError_t e = hipMemcpy(stage, sd->leaf_density, np * sizeof(float), hipMemcpyHostToDevice);
      if (e == hipSuccess) e = cvr::launch_to_half(stage, c->d_leaf_density, np, c->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
      if (e == hipSuccess && c->d_leaf_albedo) {
        e = hipMemcpy(stage, sd->leaf_albedo, np * sizeof(float4), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = cvr::launch_to_half(stage, c->d_leaf_albedo, 4 * np, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
      }
      (void)hipFree(stage);
      if (e != hipSuccess) return set_err(&c->err, CVR_ERR_HIP, "half medium upload: %s", hipGetErrorString(e));
    } else if (np) {
      HIP_TRY(c, hipMemcpy(c->d_leaf_density, sd->leaf_density, np * sizeof(float), hipMemcpyHostToDevice));
      if (c->d_leaf_albedo)
        HIP_TRY(c, hipMemcpy(c->d_leaf_albedo, sd->leaf_albedo, np * sizeof(float4), hipMemcpyHostToDevice));
    }
    return CVR_OK;
  };
  return finish_sparse(c, b, tmp, tm, refuse_overflow, upload);
}

int cvr_set_medium_device(cvr_ctx* c, const cvr_device_medium_desc* d) {
  if (!c || !d) return set_err(c ? &c->err : nullptr, CVR_ERR_INVALID, "NULL argument");
  CVR_NOT_IN_SESSION(c, "cvr_set_medium_device");
  const uint32_t* res = d->res;
  const bool sparse = (d->flags & CVR_DEVMED_SPARSE) != 0, konst = (d->flags & CVR_DEVMED_CONST_ALBEDO) != 0;
  // the host calls' shape guards, from res alone
  SparseBuild b{};
  int r = sparse ? sparse_shape_check(c, res, &b.g) : dense_shape_check(c, res, (uint32_t)c->medium_format);
  if (r) return r;
  // then the flags and the pointers
  if (d->flags & ~(uint32_t)(CVR_DEVMED_SPARSE | CVR_DEVMED_CONST_ALBEDO | CVR_DEVMED_MAX_DENSITY))
    return set_err(&c->err, CVR_ERR_INVALID, "unknown cvr_device_medium_desc flags 0x%x", d->flags);
  if (!d->d_density || (!konst && !d->d_albedo)) return set_err(&c->err, CVR_ERR_INVALID, "d_density/d_albedo is NULL");
  if (konst && d->d_albedo)
    return set_err(&c->err, CVR_ERR_INVALID, "d_albedo must be NULL with CVR_DEVMED_CONST_ALBEDO");
  if ((r = ensure_device(c))) return r;
  if (!device_readable(c, d->d_density) || (!konst && !device_readable(c, d->d_albedo)))
    return set_err(&c->err, CVR_ERR_INVALID, "d_density/d_albedo is not device-accessible memory of device %d",
                   c->device);
  if (((uintptr_t)d->d_density & 3u) || ((uintptr_t)d->d_albedo & 15u))
    return set_err(&c->err, CVR_ERR_INVALID, "d_density must be 4-byte and d_albedo 16-byte aligned");
  cvr::VoxelSource src;
  src.density = d->d_density;
  src.albedo = d->d_albedo;
  DevTemps tmp;
  return build_from_device(c, {view_of(*d), d->flags, d->const_albedo, d->max_density, nullptr}, src, b, tmp);
}

int cvr_classify_host(const void* scalar, uint32_t scalar_type, size_t n_voxels, const cvr_transfer_desc* t,
                      float* density, float* albedo) {
  if (!t || (n_voxels && !scalar)) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  if (scalar_type > CVR_SCALAR_I16) return set_err(nullptr, CVR_ERR_INVALID, "unknown scalar_type %u", scalar_type);
  if (int r = transfer_check(nullptr, t, [] { return CVR_OK; })) return r;
  const cvr::TransferParams p{t->n, t->flags, t->lo, t->hi};
  // (the table as float4: copied, the caller's need not be 16-byte aligned)
  std::vector<float4> table(t->n);
  memcpy(table.data(), t->table, (size_t)t->n * sizeof(float4));
  for (size_t i = 0; i < n_voxels; ++i) {
    const float4 e = cvr::transfer_classify(cvr::scalar_voxel(scalar, scalar_type, i), table.data(), p);
    if (density) density[i] = e.w;
    if (albedo) albedo[4 * i] = e.x, albedo[4 * i + 1] = e.y, albedo[4 * i + 2] = e.z, albedo[4 * i + 3] = 1.0f;
  }
  return CVR_OK;
}

int cvr_set_medium_scalar(cvr_ctx* c, const cvr_scalar_medium_desc* d) {
  if (!c || !d) return set_err(c ? &c->err : nullptr, CVR_ERR_INVALID, "NULL argument");
  CVR_NOT_IN_SESSION(c, "cvr_set_medium_scalar");
  const uint32_t* res = d->res;
  const bool sparse = (d->flags & CVR_DEVMED_SPARSE) != 0;
  SparseBuild b{};
  int r = sparse ? sparse_shape_check(c, res, &b.g) : dense_shape_check(c, res, (uint32_t)c->medium_format);
  if (r) return r;
  if (d->flags & ~(uint32_t)(CVR_DEVMED_SPARSE | CVR_DEVMED_MAX_DENSITY))
    return set_err(&c->err, CVR_ERR_INVALID, "unknown cvr_scalar_medium_desc flags 0x%x", d->flags);
  if (d->scalar_type > CVR_SCALAR_I16)
    return set_err(&c->err, CVR_ERR_INVALID, "unknown scalar_type %u", d->scalar_type);
  const cvr_transfer_desc* t = &d->transfer;
  r = transfer_check(&c->err, t, [&]() -> int {
    return d->d_scalar ? CVR_OK : set_err(&c->err, CVR_ERR_INVALID, "d_scalar is NULL");
  });
  if (r) return r;
  if ((r = ensure_device(c))) return r;
  if (!device_readable(c, d->d_scalar))
    return set_err(&c->err, CVR_ERR_INVALID, "d_scalar is not device-accessible memory of device %d", c->device);
  const size_t size = d->scalar_type == CVR_SCALAR_U8 ? 1 : d->scalar_type == CVR_SCALAR_F32 ? 4 : 2;
  if ((uintptr_t)d->d_scalar & (size - 1))
    return set_err(&c->err, CVR_ERR_INVALID, "d_scalar must be %zu-byte aligned", size);
  // the table goes to the device once; the kernels stage it in LDS per workgroup
  DevTemps tmp;
  float4* d_table = nullptr;
  HIP_TRY(c, tmp.alloc((void**)&d_table, (size_t)t->n * sizeof(float4)));
  HIP_TRY(c, hipMemcpy(d_table, t->table, (size_t)t->n * sizeof(float4), hipMemcpyHostToDevice));
  std::vector<float4> table(t->n);
  memcpy(table.data(), t->table, (size_t)t->n * sizeof(float4));
  cvr::VoxelSource src;
  src.scalar = d->d_scalar;
  src.scalar_type = d->scalar_type;
  src.table = d_table;
  src.tf = {t->n, t->flags, t->lo, t->hi};
  return build_from_device(c, {view_of(*d), d->flags, nullptr, d->max_density, &table[0].x}, src, b, tmp);
}

int cvr_classify_labels_host(const void* scalar, uint32_t scalar_type, const uint8_t* labels, size_t n_voxels,
                             const cvr_label_transfer_desc* t, float* density, float* albedo, uint64_t* counts) {
  if (!t || (n_voxels && (!scalar || !labels))) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  if (scalar_type > CVR_SCALAR_I16) return set_err(nullptr, CVR_ERR_INVALID, "unknown scalar_type %u", scalar_type);
  if (int r = label_transfer_check(nullptr, t, [] { return CVR_OK; })) return r;
  const cvr::TransferParams p{t->n, t->flags, t->lo, t->hi};
  // (the table as float4: copied, the caller's need not be 16-byte aligned)
  std::vector<float4> table((size_t)t->n * t->m);
  memcpy(table.data(), t->table, table.size() * sizeof(float4));
  if (counts) memset(counts, 0, 256 * sizeof(uint64_t));
  for (size_t i = 0; i < n_voxels; ++i) {
    const float4 e = cvr::label_classify(cvr::scalar_voxel(scalar, scalar_type, i), labels[i], table.data(), t->m, p);
    if (density) density[i] = e.w;
    if (albedo) albedo[4 * i] = e.x, albedo[4 * i + 1] = e.y, albedo[4 * i + 2] = e.z, albedo[4 * i + 3] = 1.0f;
    if (counts) ++counts[labels[i]];
  }
  return CVR_OK;
}

int cvr_set_medium_labeled(cvr_ctx* c, const cvr_labeled_medium_desc* d) {
  if (!c || !d) return set_err(c ? &c->err : nullptr, CVR_ERR_INVALID, "NULL argument");
  CVR_NOT_IN_SESSION(c, "cvr_set_medium_labeled");
  const uint32_t* res = d->res;
  const bool sparse = (d->flags & CVR_DEVMED_SPARSE) != 0;
  SparseBuild b{};
  int r = sparse ? sparse_shape_check(c, res, &b.g) : dense_shape_check(c, res, (uint32_t)c->medium_format);
  if (r) return r;
  if (d->flags & ~(uint32_t)(CVR_DEVMED_SPARSE | CVR_DEVMED_MAX_DENSITY))
    return set_err(&c->err, CVR_ERR_INVALID, "unknown cvr_labeled_medium_desc flags 0x%x", d->flags);
  if (d->scalar_type > CVR_SCALAR_I16)
    return set_err(&c->err, CVR_ERR_INVALID, "unknown scalar_type %u", d->scalar_type);
  const cvr_label_transfer_desc* t = &d->transfer;
  r = label_transfer_check(&c->err, t, [&]() -> int {
    return d->d_scalar && d->d_labels ? CVR_OK : set_err(&c->err, CVR_ERR_INVALID, "d_scalar/d_labels is NULL");
  });
  if (r) return r;
  if ((r = ensure_device(c))) return r;
  if (!device_readable(c, d->d_scalar))
    return set_err(&c->err, CVR_ERR_INVALID, "d_scalar is not device-accessible memory of device %d", c->device);
  const size_t size = d->scalar_type == CVR_SCALAR_U8 ? 1 : d->scalar_type == CVR_SCALAR_F32 ? 4 : 2;
  if ((uintptr_t)d->d_scalar & (size - 1))
    return set_err(&c->err, CVR_ERR_INVALID, "d_scalar must be %zu-byte aligned", size);
  if (!device_readable(c, d->d_labels))
    return set_err(&c->err, CVR_ERR_INVALID, "d_labels is not device-accessible memory of device %d", c->device);
  // the table goes to the device once; the kernels stage it in LDS per workgroup
  const size_t entries = (size_t)t->n * t->m;
  DevTemps tmp;
  float4* d_table = nullptr;
  HIP_TRY(c, tmp.alloc((void**)&d_table, entries * sizeof(float4)));
  HIP_TRY(c, hipMemcpy(d_table, t->table, entries * sizeof(float4), hipMemcpyHostToDevice));
  std::vector<float4> table(entries);
  memcpy(table.data(), t->table, entries * sizeof(float4));
  cvr::VoxelSource src;
  src.scalar = d->d_scalar;
  src.scalar_type = d->scalar_type;
  src.table = d_table;
  src.tf = {t->n, t->flags, t->lo, t->hi};
  src.labels = static_cast<const uint8_t*>(d->d_labels);
  src.label_rows = t->m;
  memcpy(src.res, res, sizeof(src.res));
  return build_from_device(c, {view_of(*d), d->flags, nullptr, d->max_density, &table[0].x}, src, b, tmp);
}

int cvr_medium_label_info(const cvr_ctx* c, uint32_t* m, uint64_t counts[256]) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  if (!c->have_medium) return set_err(nullptr, CVR_ERR_STATE, "no medium");
  if (m) *m = c->medium_label_rows;
  if (counts) memcpy(counts, c->medium_label_counts, sizeof(c->medium_label_counts));
  return CVR_OK;
}

int cvr_set_medium_scene_labels(cvr_ctx* c, const cvr_scene* scene, const cvr_label_transfer_desc* t,
                                const uint8_t* host_labels, size_t n_labels, uint32_t flags) {
  if (!c || !scene || !t) return set_err(c ? &c->err : nullptr, CVR_ERR_INVALID, "NULL argument");
  const uint8_t* bytes = nullptr;
  size_t n = 0;
  cvr_medium_desc md{};
  int r = cvr_scene_raw_bytes(scene, &bytes, &n);
  if (!r) r = cvr_scene_medium(scene, &md);
  if (r || !n || n != (size_t)md.res[0] * md.res[1] * md.res[2])
    return set_err(&c->err, CVR_ERR_INVALID, "the scene has no raw bytes (one per voxel): not a Raw scene");
  if (!host_labels || n_labels != n)
    return set_err(&c->err, CVR_ERR_INVALID, "%zu labels for a scene of %zu voxels (one byte per voxel)",
                   host_labels ? n_labels : (size_t)0, n);
  if ((r = ensure_device(c))) return r;
  DevTemps tmp;
  void *d_bytes = nullptr, *d_labels = nullptr;
  HIP_TRY(c, tmp.alloc(&d_bytes, n));
  HIP_TRY(c, tmp.alloc(&d_labels, n));
  HIP_TRY(c, hipMemcpy(d_bytes, bytes, n, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(d_labels, host_labels, n, hipMemcpyHostToDevice));
  cvr_labeled_medium_desc d{};
  memcpy(d.res, md.res, sizeof(d.res));
  d.flags = flags | CVR_DEVMED_MAX_DENSITY;
  d.d_scalar = d_bytes;
  d.scalar_type = CVR_SCALAR_U8;
  d.d_labels = d_labels;
  d.transfer = *t;
  d.transfer.lo = 0.0f;
  d.transfer.hi = (float)*std::max_element(bytes, bytes + n);
  memcpy(d.box_min, md.box_min, sizeof(d.box_min));
  memcpy(d.box_max, md.box_max, sizeof(d.box_max));
  d.scale = md.scale;
  d.g = md.g;
  d.roughness[0] = md.roughness[0], d.roughness[1] = md.roughness[1];
  d.eta = md.eta;
  return cvr_set_medium_labeled(c, &d);
}

int cvr_classify_gradient_host(const void* scalar, uint32_t scalar_type, const uint32_t res[3],
                               const cvr_gradient_transfer_desc* t, float* density, float* albedo,
                               float* gradient_magnitude) {
  if (!t || !res) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  const uint32_t nx = res[0], ny = res[1], nz = res[2];
  const size_t n_voxels = (size_t)nx * ny * nz;
  if (n_voxels && !scalar) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  if (scalar_type > CVR_SCALAR_I16) return set_err(nullptr, CVR_ERR_INVALID, "unknown scalar_type %u", scalar_type);
  cvr::GradientParams p;
  if (int r = gradient_check(nullptr, t, [] { return CVR_OK; }, &p)) return r;
  // (the table as float4: copied, the caller's need not be 16-byte aligned)
  std::vector<float4> table((size_t)t->n * t->m);
  memcpy(table.data(), t->table, table.size() * sizeof(float4));
  cvr::gradient_for_each([&](size_t i) { return cvr::scalar_voxel(scalar, scalar_type, i); }, res, p.axes,
                         [&](size_t i, float s, float mag) {
                           const float4 e = cvr::gradient_classify(s, mag, table.data(), p);
                           if (density) density[i] = e.w;
                           if (albedo)
                             albedo[4 * i] = e.x, albedo[4 * i + 1] = e.y, albedo[4 * i + 2] = e.z, albedo[4 * i + 3] = 1.0f;
                           if (gradient_magnitude) gradient_magnitude[i] = mag;
                         });
  return CVR_OK;
}

int cvr_set_medium_gradient(cvr_ctx* c, const cvr_gradient_medium_desc* d) {
  if (!c || !d) return set_err(c ? &c->err : nullptr, CVR_ERR_INVALID, "NULL argument");
  CVR_NOT_IN_SESSION(c, "cvr_set_medium_gradient");
  const uint32_t* res = d->res;
  const bool sparse = (d->flags & CVR_DEVMED_SPARSE) != 0;
  SparseBuild b{};
  int r = sparse ? sparse_shape_check(c, res, &b.g) : dense_shape_check(c, res, (uint32_t)c->medium_format);
  if (r) return r;
  if (d->flags & ~(uint32_t)(CVR_DEVMED_SPARSE | CVR_DEVMED_MAX_DENSITY))
    return set_err(&c->err, CVR_ERR_INVALID, "unknown cvr_gradient_medium_desc flags 0x%x", d->flags);
  if (d->scalar_type > CVR_SCALAR_I16)
    return set_err(&c->err, CVR_ERR_INVALID, "unknown scalar_type %u", d->scalar_type);
  const cvr_gradient_transfer_desc* t = &d->transfer;
  cvr::VoxelSource src;
  r = gradient_check(&c->err, t, [&]() -> int {
    return d->d_scalar ? CVR_OK : set_err(&c->err, CVR_ERR_INVALID, "d_scalar is NULL");
  }, &src.gtf);
  if (r) return r;
  if ((r = ensure_device(c))) return r;
  if (!device_readable(c, d->d_scalar))
    return set_err(&c->err, CVR_ERR_INVALID, "d_scalar is not device-accessible memory of device %d", c->device);
  const size_t size = d->scalar_type == CVR_SCALAR_U8 ? 1 : d->scalar_type == CVR_SCALAR_F32 ? 4 : 2;
  if ((uintptr_t)d->d_scalar & (size - 1))
    return set_err(&c->err, CVR_ERR_INVALID, "d_scalar must be %zu-byte aligned", size);
  // the table goes to the device once; the kernels stage it in LDS per workgroup
  const size_t entries = (size_t)t->n * t->m;
  DevTemps tmp;
  float4* d_table = nullptr;
  HIP_TRY(c, tmp.alloc((void**)&d_table, entries * sizeof(float4)));
  HIP_TRY(c, hipMemcpy(d_table, t->table, entries * sizeof(float4), hipMemcpyHostToDevice));
  std::vector<float4> table(entries);
  memcpy(table.data(), t->table, entries * sizeof(float4));
  src.scalar = d->d_scalar;
  src.scalar_type = d->scalar_type;
  src.table = d_table;
  src.gradient = true;
  memcpy(src.res, res, sizeof(src.res));
  return build_from_device(c, {view_of(*d), d->flags, nullptr, d->max_density, &table[0].x}, src, b, tmp);
}

int cvr_set_medium_scene_gradient(cvr_ctx* c, const cvr_scene* scene, const cvr_gradient_transfer_desc* t,
                                  uint32_t flags) {
  if (!c || !scene || !t) return set_err(c ? &c->err : nullptr, CVR_ERR_INVALID, "NULL argument");
  const uint8_t* bytes = nullptr;
  size_t n = 0;
  cvr_medium_desc md{};
  int r = cvr_scene_raw_bytes(scene, &bytes, &n);
  if (!r) r = cvr_scene_medium(scene, &md);
  if (r || !n || n != (size_t)md.res[0] * md.res[1] * md.res[2])
    return set_err(&c->err, CVR_ERR_INVALID, "the scene has no raw bytes (one per voxel): not a Raw scene");
  if ((r = ensure_device(c))) return r;
  DevTemps tmp;
  void* d_bytes = nullptr;
  HIP_TRY(c, tmp.alloc(&d_bytes, n));
  HIP_TRY(c, hipMemcpy(d_bytes, bytes, n, hipMemcpyHostToDevice));
  cvr_gradient_medium_desc d{};
  memcpy(d.res, md.res, sizeof(d.res));
  d.flags = flags | CVR_DEVMED_MAX_DENSITY;
  d.d_scalar = d_bytes;
  d.scalar_type = CVR_SCALAR_U8;
  d.transfer = *t;
  d.transfer.lo = 0.0f;
  d.transfer.hi = (float)*std::max_element(bytes, bytes + n);
  memcpy(d.box_min, md.box_min, sizeof(d.box_min));
  memcpy(d.box_max, md.box_max, sizeof(d.box_max));
  d.scale = md.scale;
  d.g = md.g;
  d.roughness[0] = md.roughness[0], d.roughness[1] = md.roughness[1];
  d.eta = md.eta;
  return cvr_set_medium_gradient(c, &d);
}

int cvr_set_medium_scene_transfer(cvr_ctx* c, const cvr_scene* scene, const cvr_transfer_desc* t, uint32_t flags) {
  if (!c || !scene || !t) return set_err(c ? &c->err : nullptr, CVR_ERR_INVALID, "NULL argument");
  const uint8_t* bytes = nullptr;
  size_t n = 0;
  cvr_medium_desc md{};
  int r = cvr_scene_raw_bytes(scene, &bytes, &n);
  if (!r) r = cvr_scene_medium(scene, &md);
  if (r || !n || n != (size_t)md.res[0] * md.res[1] * md.res[2])
    return set_err(&c->err, CVR_ERR_INVALID, "the scene has no raw bytes (one per voxel): not a Raw scene");
  if ((r = ensure_device(c))) return r;
  DevTemps tmp;
  void* d_bytes = nullptr;
  HIP_TRY(c, tmp.alloc(&d_bytes, n));
  HIP_TRY(c, hipMemcpy(d_bytes, bytes, n, hipMemcpyHostToDevice));
  cvr_scalar_medium_desc d{};
  memcpy(d.res, md.res, sizeof(d.res));
  d.flags = flags | CVR_DEVMED_MAX_DENSITY;
  d.d_scalar = d_bytes;
  d.scalar_type = CVR_SCALAR_U8;
  d.transfer = *t;
  d.transfer.lo = 0.0f;
  d.transfer.hi = (float)*std::max_element(bytes, bytes + n);
  memcpy(d.box_min, md.box_min, sizeof(d.box_min));
  memcpy(d.box_max, md.box_max, sizeof(d.box_max));
  d.scale = md.scale;
  d.g = md.g;
  d.roughness[0] = md.roughness[0], d.roughness[1] = md.roughness[1];
  d.eta = md.eta;
  return cvr_set_medium_scalar(c, &d);
}

int cvr_debug_device_medium_ms(const cvr_ctx* c, double out[6]) {
  if (!c || !out) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  for (int i = 0; i < 6; ++i) out[i] = c->devmed_ms[i];
  return CVR_OK;
}

int cvr_debug_build_geometry(uint32_t out[16]) {
  if (!out) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  const uint32_t g[] = {cvr::kScanGridCap,   cvr::kStreamGridCap,    cvr::kScanTile,
                        cvr::kScanSumsChunk, cvr::kWalkTaskCap,      cvr::kWalkZ,
                        cvr::kLeafRunVoxels, cvr::kLeafRunLeaves,    cvr::kLeafFlagsGridCap,
                        cvr::kToHalfGridCap, cvr::kBuildCellsGrid,   cvr::kBuildBoundsGrid,
                        cvr::kBuildSparseCellsGrid, cvr::kBuildSparseBoundsGrid};
  constexpr uint32_t n = sizeof(g) / sizeof(g[0]);
  static_assert(n < 16, "the last slot holds the count");
  for (uint32_t i = 0; i < 16; ++i) out[i] = i < n ? g[i] : 0u;
  out[15] = n;
  return CVR_OK;
}

int cvr_debug_copy_medium(const cvr_ctx* c, int which, void* host_dst, size_t bytes, size_t* needed) {
  if (!c || !needed) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  *needed = 0;
  if (!c->have_medium) return set_err(nullptr, CVR_ERR_STATE, "no medium");
  if (which < 0 || which >= CVR_MEDIUM_ARRAY_COUNT)
    return set_err(nullptr, CVR_ERR_INVALID, "unknown medium array %d", which);
  // (a shared medium: m and minfo are the source's, so the arrays are too)
  const cvr::MediumParams& m = c->m;
  const bool sparse = m.leaves != nullptr;
  const size_t nleaf = sparse ? (size_t)m.lnx * m.lny * ((m.rz + 7u) / 8u) : 0;
  const uint32_t S = 1u << m.bshift;
  const size_t nwords = sparse ? (size_t)m.bnxy * ((m.rz + S - 1) / S) + 1 : 0;
  // the leaf pools hold 512 voxels per leaf (the density pool's allocation is one voxel when there is no leaf)
  const size_t np = sparse ? c->minfo.density_bytes / (512u * (m.format ? 2u : 4u)) * 512u : 0;
  const void* src = nullptr;
  size_t n = 0;
  switch (which) {
    case CVR_MEDIUM_DENSITY: if (!sparse) src = m.density, n = c->minfo.density_bytes; break;
    case CVR_MEDIUM_ALBEDO: if (!sparse) src = m.albedo, n = c->minfo.albedo_bytes; break;
    case CVR_MEDIUM_CELLS: if (!sparse) src = m.cells, n = c->minfo.cells_bytes; break;
    case CVR_MEDIUM_BOUNDS: if (!sparse) src = m.bounds, n = c->minfo.bounds_bytes; break;
    case CVR_MEDIUM_LEAF_TABLE: src = m.leaves, n = nleaf * sizeof(uint32_t); break;
    case CVR_MEDIUM_LEAF_DENSITY: if (sparse) src = m.leaf_density, n = np * (m.format ? 2u : 4u); break;
    case CVR_MEDIUM_LEAF_ALBEDO: if (sparse) src = m.leaf_albedo, n = c->minfo.albedo_bytes; break;
    case CVR_MEDIUM_CELL_SLOTS: src = m.sbounds, n = nleaf * sizeof(uint32_t); break;
    case CVR_MEDIUM_SPARSE_CELLS: if (sparse) src = m.cells, n = c->minfo.cells_bytes; break;
    case CVR_MEDIUM_BRICK_WORDS: src = m.sbounds, n = nwords * sizeof(uint32_t); break;
    case CVR_MEDIUM_MASK: src = m.emask, n = m.emask ? cvr::kEmaskWords * sizeof(uint32_t) : 0; break;
  }
  if (!src || !n) return CVR_OK;  // the medium has no such array
  *needed = n;
  if (!host_dst || bytes < n)
    return set_err(nullptr, CVR_ERR_INVALID, "cvr_debug_copy_medium: array %d holds %zu bytes, the buffer %zu", which, n,
                   bytes);
  if (hipSetDevice(c->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
    return set_err(nullptr, CVR_ERR_HIP, "cvr_debug_copy_medium: the device is not ready");
  if (which != CVR_MEDIUM_CELL_SLOTS) {
    if (hipMemcpy(host_dst, src, n, hipMemcpyDeviceToHost) != hipSuccess)
      return set_err(nullptr, CVR_ERR_HIP, "cvr_debug_copy_medium: reading array %d failed", which);
    return CVR_OK;
  }
  // a leaf's cell-leaf slot is kept in the low 24 bits of the words of its bricks: the first one's
  std::vector<uint32_t> words(nwords);
  if (hipMemcpy(words.data(), src, nwords * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
    return set_err(nullptr, CVR_ERR_HIP, "cvr_debug_copy_medium: reading array %d failed", which);
  uint32_t* slots = static_cast<uint32_t*>(host_dst);
  const uint32_t up = 3u - m.bshift, lnz = (m.rz + 7u) / 8u;
  for (uint32_t z = 0; z < lnz; ++z)
    for (uint32_t y = 0; y < m.lny; ++y)
      for (uint32_t x = 0; x < m.lnx; ++x)
        slots[((size_t)z * m.lny + y) * m.lnx + x] =
            words[((size_t)(z << up) * m.bny + (y << up)) * m.bnx + (x << up)] & 0xFFFFFFu;
  return CVR_OK;
}

int cvr_medium_layout(const cvr_ctx* c, struct cvr_medium_layout* out) {
  if (!c || !out) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  if (!c->have_medium) return set_err(nullptr, CVR_ERR_STATE, "no medium");
  const cvr::MediumParams& m = c->m;
  struct cvr_medium_layout l {};
  l.sparse = m.leaves != nullptr;
  l.albedo_uniform = m.albedo_uniform;
  if (l.sparse) {
    // (the leaf pool holds 512 voxels per leaf, one voxel when there is no leaf)
    l.n_leaves = (uint32_t)(c->minfo.density_bytes / (512u * (m.format ? 2u : 4u)));
    l.n_cell_leaves = (uint32_t)c->n_cell_leaves;
  }
  l.brick_shift = m.bshift;
  l.mask_shift = m.eshift;
  if (l.sparse || m.albedo_uniform) {
    l.albedo_bg[0] = m.albedo_bg.x;
    l.albedo_bg[1] = m.albedo_bg.y;
    l.albedo_bg[2] = m.albedo_bg.z;
  }
  if (m.emask) {
    // the medium's own mask (a shared medium: the source context's buffer)
    if (hipSetDevice(c->device) != hipSuccess ||
        hipMemcpy(l.mask, m.emask, sizeof(l.mask), hipMemcpyDeviceToHost) != hipSuccess)
      return set_err(nullptr, CVR_ERR_HIP, "cvr_medium_layout: reading the mask failed");
  }
  *out = l;
  return CVR_OK;
}

int cvr_share_medium(cvr_ctx* c, const cvr_ctx* src) {
  if (!c || !src) return set_err(c ? &c->err : nullptr, CVR_ERR_INVALID, "NULL argument");
  CVR_NOT_IN_SESSION(c, "cvr_share_medium");
  if (c == src) return CVR_OK;
  if (!src->have_medium) return set_err(&c->err, CVR_ERR_STATE, "source context has no medium");
  if (src->device != c->device)
    return set_err(&c->err, CVR_ERR_INVALID, "source context is on device %d, not %d", src->device, c->device);
  int r = ensure_device(c);
  if (r) return r;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  // drop this context's own medium; the kernels read the source's buffers
  drop_dense(c);
  free_sparse(c);
  drop_light_volume(c);
  c->m = src->m;
  c->minfo = src->minfo;
  c->n_cell_leaves = src->n_cell_leaves;
  c->medium_clipped = src->medium_clipped;
  c->medium_clip = src->medium_clip;
  c->medium_kept = src->medium_kept;
  c->medium_label_rows = src->medium_label_rows;
  memcpy(c->medium_label_counts, src->medium_label_counts, sizeof(c->medium_label_counts));
  c->have_medium = true;
  c->inited = false;
  return CVR_OK;
}

int cvr_medium_info(const cvr_ctx* c, struct cvr_medium_info* out) {
  if (!c || !out) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  if (!c->have_medium) return set_err(nullptr, CVR_ERR_STATE, "no medium");
  *out = c->minfo;
  return CVR_OK;
}

int cvr_set_clip(cvr_ctx* c, const cvr_clip_desc* d) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  CVR_NOT_IN_SESSION(c, "cvr_set_clip");
  if (int r = clip_check(&c->err, d)) return r;
  c->clip = *d;
  c->clip_set = true;
  return CVR_OK;
}

int cvr_clear_clip(cvr_ctx* c) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  CVR_NOT_IN_SESSION(c, "cvr_clear_clip");
  c->clip_set = false;
  return CVR_OK;
}

int cvr_get_clip(const cvr_ctx* c, cvr_clip_desc* d, int* set) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  if (d) *d = c->clip_set ? c->clip : clip_everything();
  if (set) *set = c->clip_set ? 1 : 0;
  return CVR_OK;
}

int cvr_clip_host(const uint32_t res[3], const cvr_clip_desc* d, float* density, float* albedo, uint8_t* keep) {
  if (!res) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  if (int r = clip_check(nullptr, d)) return r;
  const uint32_t nx = res[0], ny = res[1], nz = res[2];
  if (!nx || !ny || !nz) return set_err(nullptr, CVR_ERR_INVALID, "empty grid");
  if ((uint64_t)nx * ny > 0xFFFFFFFFull || (uint64_t)nx * ny * nz > 0xFFFFFFFFull)
    return set_err(nullptr, CVR_ERR_INVALID, "grid exceeds 2^32 voxels");
  cvr::ClipRegion r{};
  for (int a = 0; a < 3; ++a) {
    r.lo[a] = d->lo[a];
    r.hi[a] = std::min(d->hi[a], res[a]);
  }
  r.n_planes = d->n_planes;
  memcpy(r.planes, d->planes, sizeof(r.planes));
  // (voxel 0's albedo before voxel 0 itself may be overwritten with it)
  float a0[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (albedo) memcpy(a0, albedo, sizeof(a0));
  size_t i = 0;
  for (uint32_t z = 0; z < nz; ++z)
    for (uint32_t y = 0; y < ny; ++y)
      for (uint32_t x = 0; x < nx; ++x, ++i) {
        const bool k = cvr::clip_keeps(r, x, y, z);
        if (keep) keep[i] = k ? 1 : 0;
        if (k) continue;
        if (density) density[i] = 0.0f;
        if (albedo) memcpy(albedo + 4 * i, a0, sizeof(a0));
      }
  return CVR_OK;
}

int cvr_medium_clip_info(const cvr_ctx* c, cvr_clip_desc* d, uint64_t* kept) {
  if (!c) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  if (!c->have_medium) return set_err(nullptr, CVR_ERR_STATE, "no medium");
  if (d) *d = c->medium_clipped ? c->medium_clip : clip_everything();
  if (kept) *kept = c->medium_clipped ? c->medium_kept : (uint64_t)c->m.rx * c->m.ry * c->m.rz;
  return CVR_OK;
}

int cvr_half_round(const float* in, float* out, size_t n) {
  if (n && (!in || !out)) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  for (size_t i = 0; i < n; ++i) out[i] = half_round1(in[i]);
  return CVR_OK;
}

}  // extern "C"
