// cvr_field_api.cpp - C ABI of the field statistics and value-gradient histograms (cvr.h,
// CVR_HAS_FIELD_HISTOGRAM): the host statements on a field in host memory and the device passes on
// one in device memory.  The context supplies the device and the stream and is otherwise only
// read.  The per-voxel definitions: cvr_kernels.h, cvr_gradient.h; the kernels: cvr_field.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "cvr_ctx.h"

using cvr::set_err;

namespace {

size_t scalar_size(uint32_t type) { return type == CVR_SCALAR_U8 ? 1 : type == CVR_SCALAR_F32 ? 4 : 2; }

// The refusals of cvr.h in their order, rules 2 to 8 (rule 1, the NULL arguments, is the entry
// point's; rule 9 needs the device).  h null: the statistics, which always take the gradient.
// `counts`: the histogram's output pointer, judged with the scalar pointer (rule 8).
int field_check(std::string* err, const cvr_field_desc* f, const cvr_histogram_desc* h, const void* counts) {
  const uint64_t voxels = (uint64_t)f->res[0] * f->res[1];  // < 2^64
  if (f->res[0] == 0 || f->res[1] == 0 || f->res[2] == 0) return set_err(err, CVR_ERR_INVALID, "empty field");
  if (voxels > 0xFFFFFFFFull || voxels * f->res[2] > 0xFFFFFFFFull)
    return set_err(err, CVR_ERR_INVALID, "field of %u x %u x %u voxels: more than 2^32 - 1", f->res[0], f->res[1],
                   f->res[2]);
  if (f->scalar_type > CVR_SCALAR_I16) return set_err(err, CVR_ERR_INVALID, "unknown scalar_type %u", f->scalar_type);
  if (f->reserved) return set_err(err, CVR_ERR_INVALID, "cvr_field_desc reserved 0x%x: must be 0", f->reserved);
  bool gradient = true;
  if (h) {
    if (h->flags || h->reserved)
      return set_err(err, CVR_ERR_INVALID, "cvr_histogram_desc flags 0x%x, reserved 0x%x: both must be 0", h->flags,
                     h->reserved);
    if (h->n < 2u || h->m < 1u || (uint64_t)h->n * h->m > cvr::kFieldMaxBins)
      return set_err(err, CVR_ERR_INVALID, "histogram of %u x %u bins (n >= 2, m >= 1, n * m <= %u)", h->n, h->m,
                     cvr::kFieldMaxBins);
    if (!std::isfinite(h->lo) || !std::isfinite(h->hi) || !(h->hi > h->lo))
      return set_err(err, CVR_ERR_INVALID, "value range lo %g, hi %g: both finite and hi > lo", (double)h->lo,
                     (double)h->hi);
    gradient = h->m > 1u;
    if (gradient && (!std::isfinite(h->glo) || !std::isfinite(h->ghi) || !(h->glo >= 0.0f) || !(h->ghi > h->glo)))
      return set_err(err, CVR_ERR_INVALID, "gradient range glo %g, ghi %g: both finite, glo >= 0 and ghi > glo",
                     (double)h->glo, (double)h->ghi);
  }
  if (gradient)
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(f->spacing[k]) || !(f->spacing[k] > 0.0f))
        return set_err(err, CVR_ERR_INVALID, "voxel spacing[%d] = %g: finite and > 0", k, (double)f->spacing[k]);
  if (!f->scalar) return set_err(err, CVR_ERR_INVALID, "scalar is NULL");
  if (h && !counts) return set_err(err, CVR_ERR_INVALID, "counts is NULL");
  return CVR_OK;
}

int aligned_check(std::string* err, const cvr_field_desc* f) {
  const size_t size = scalar_size(f->scalar_type);
  if ((uintptr_t)f->scalar & (size - 1)) return set_err(err, CVR_ERR_INVALID, "scalar must be %zu-byte aligned", size);
  return CVR_OK;
}

// The field as the kernels and the host loops take it (gradient false: the factors stay 1, 0.5
// and are not read)
cvr::FieldSrc source_of(const cvr_field_desc* f, bool gradient) {
  cvr::FieldSrc s;
  s.scalar = f->scalar;
  s.scalar_type = f->scalar_type;
  memcpy(s.res, f->res, sizeof(s.res));
  if (gradient) s.axes = cvr::gradient_axes(f->spacing);
  return s;
}

cvr::FieldBins bins_of(const cvr_histogram_desc* h) {
  return cvr::FieldBins{h->n, h->m, h->lo, h->hi, h->m > 1u ? h->glo : 0.0f, h->m > 1u ? h->ghi : 1.0f};
}

// fn(i, s, mag) for every voxel of a host field, x fastest: the statement's loop
template <class F>
void for_each_voxel(const cvr::FieldSrc& s, F fn) {
  cvr::gradient_for_each([&](size_t i) { return cvr::scalar_voxel(s.scalar, s.scalar_type, i); }, s.res, s.axes, fn);
}

void stats_from_scan(const cvr::FieldScan& sc, struct cvr_field_stats* out) {
  const uint32_t lo = cvr::field_unkey(sc.kmin), hi = cvr::field_unkey(sc.kmax);
  memset(out, 0, sizeof(*out));
  memcpy(&out->vmin, &lo, 4);
  memcpy(&out->vmax, &hi, 4);
  memcpy(&out->gmax, &sc.gmax_bits, 4);
  out->nan_values = sc.nan_values;
  out->nan_gradients = sc.nan_gradients;
}

const cvr::FieldScan kEmptyScan{cvr::kFieldKeyPosInf, cvr::kFieldKeyNegInf, 0u, 0u, 0ull, 0ull};

// Rule 9 for one pointer
int device_check(cvr_ctx* c, const void* p, size_t align, const char* name) {
  if (!cvr::device_readable(c, p))
    return set_err(&c->err, CVR_ERR_INVALID, "%s is not device-accessible memory of device %d", name, c->device);
  if ((uintptr_t)p & (align - 1)) return set_err(&c->err, CVR_ERR_INVALID, "%s must be %zu-byte aligned", name, align);
  return CVR_OK;
}

}  // namespace

extern "C" {

int cvr_field_stats_host(const cvr_field_desc* f, struct cvr_field_stats* out) {
  if (!f || !out) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  if (int r = field_check(nullptr, f, nullptr, nullptr)) return r;
  if (int r = aligned_check(nullptr, f)) return r;
  cvr::FieldScan sc = kEmptyScan;
  for_each_voxel(source_of(f, true), [&](size_t, float s, float mag) {
    if (s == s) {
      uint32_t bits;
      memcpy(&bits, &s, 4);
      const uint32_t k = cvr::field_key(bits);
      sc.kmin = k < sc.kmin ? k : sc.kmin;
      sc.kmax = k > sc.kmax ? k : sc.kmax;
    } else {
      ++sc.nan_values;
    }
    if (mag == mag) {
      uint32_t bits;
      memcpy(&bits, &mag, 4);
      sc.gmax_bits = bits > sc.gmax_bits ? bits : sc.gmax_bits;
    } else {
      ++sc.nan_gradients;
    }
  });
  stats_from_scan(sc, out);
  return CVR_OK;
}

int cvr_field_histogram_host(const cvr_field_desc* f, const cvr_histogram_desc* h, uint32_t* counts) {
  if (!f || !h) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  if (int r = field_check(nullptr, f, h, counts)) return r;
  if (int r = aligned_check(nullptr, f)) return r;
  const cvr::FieldBins b = bins_of(h);
  memset(counts, 0, (size_t)b.n * b.m * sizeof(uint32_t));
  if (b.m > 1u) {
    for_each_voxel(source_of(f, true), [&](size_t, float s, float mag) {
      const uint32_t i = cvr::field_bin(cvr::unit_clamp(s, b.lo, b.hi), b.n);
      const uint32_t j = cvr::field_bin(cvr::unit_clamp(mag, b.glo, b.ghi), b.m);
      ++counts[(size_t)j * b.n + i];
    });
  } else {
    const size_t voxels = (size_t)f->res[0] * f->res[1] * f->res[2];
    for (size_t v = 0; v < voxels; ++v)
      ++counts[cvr::field_bin(cvr::unit_clamp(cvr::scalar_voxel(f->scalar, f->scalar_type, v), b.lo, b.hi), b.n)];
  }
  return CVR_OK;
}

int cvr_field_stats(cvr_ctx* c, const cvr_field_desc* f, struct cvr_field_stats* out) {
  if (!c || !f || !out) return set_err(c ? &c->err : nullptr, CVR_ERR_INVALID, "NULL argument");
  int r = field_check(&c->err, f, nullptr, nullptr);
  if (r) return r;
  if ((r = cvr::ensure_device(c))) return r;
  if ((r = device_check(c, f->scalar, scalar_size(f->scalar_type), "scalar"))) return r;
  cvr::FieldScan* d_scan = nullptr;
  HIP_TRY(c, hipMalloc((void**)&d_scan, sizeof(cvr::FieldScan)));
  cvr::FieldScan sc = kEmptyScan;
  hipError_t e = hipMemcpyAsync(d_scan, &sc, sizeof(sc), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = cvr::launch_field_stats(source_of(f, true), d_scan, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(&sc, d_scan, sizeof(sc), hipMemcpyDeviceToHost, c->stream);
  const hipError_t es = hipStreamSynchronize(c->stream);
  (void)hipFree(d_scan);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return set_err(&c->err, CVR_ERR_HIP, "cvr_field_stats: %s", hipGetErrorString(e));
  stats_from_scan(sc, out);
  return CVR_OK;
}

int cvr_field_histogram_buffers(cvr_ctx* c, const cvr_field_desc* f, const cvr_histogram_desc* h, uint32_t* d_counts) {
  if (!c || !f || !h) return set_err(c ? &c->err : nullptr, CVR_ERR_INVALID, "NULL argument");
  int r = field_check(&c->err, f, h, d_counts);
  if (r) return r;
  if ((r = cvr::ensure_device(c))) return r;
  if ((r = device_check(c, f->scalar, scalar_size(f->scalar_type), "scalar"))) return r;
  if ((r = device_check(c, d_counts, sizeof(uint32_t), "d_counts"))) return r;
  HIP_TRY(c, cvr::launch_field_histogram(source_of(f, h->m > 1u), bins_of(h), d_counts, c->stream));
  return CVR_OK;
}

int cvr_field_histogram(cvr_ctx* c, const cvr_field_desc* f, const cvr_histogram_desc* h, uint32_t* host_counts) {
  if (!c || !f || !h) return set_err(c ? &c->err : nullptr, CVR_ERR_INVALID, "NULL argument");
  int r = field_check(&c->err, f, h, host_counts);
  if (r) return r;
  if ((r = cvr::ensure_device(c))) return r;
  if ((r = device_check(c, f->scalar, scalar_size(f->scalar_type), "scalar"))) return r;
  const size_t bytes = (size_t)h->n * h->m * sizeof(uint32_t);
  uint32_t* d_counts = nullptr;
  HIP_TRY(c, hipMalloc((void**)&d_counts, bytes));
  hipError_t e = cvr::launch_field_histogram(source_of(f, h->m > 1u), bins_of(h), d_counts, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(host_counts, d_counts, bytes, hipMemcpyDeviceToHost, c->stream);
  const hipError_t es = hipStreamSynchronize(c->stream);
  (void)hipFree(d_counts);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return set_err(&c->err, CVR_ERR_HIP, "cvr_field_histogram: %s", hipGetErrorString(e));
  return CVR_OK;
}

int cvr_debug_field_geometry(uint32_t out[8]) {
  if (!out) return set_err(nullptr, CVR_ERR_INVALID, "NULL argument");
  const uint32_t v[8] = {cvr::kWalkTaskCap, cvr::kWalkZ, cvr::kFieldGrid1D, cvr::kFieldLdsBins, cvr::kFieldMaxBins,
                         0u, 0u, 5u};
  memcpy(out, v, sizeof(v));
  return CVR_OK;
}

}  // extern "C"
