// cvr_image_io.cpp - cvr_read_image / cvr_free_image (cvr.h): Radiance .hdr and colour .pfm files
// into RGB floats, row 0 the top.  Plain C++ with no HIP include, so that a host compiler builds it
// alone (tests/cpp/image_io_san.cpp runs it under the host sanitizers).  Every read goes through
// one bounds-checked cursor over the file's bytes; nothing is allocated from a header's numbers
// before they have been held against the bytes that are there.
#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "cvr.h"

namespace {

struct Cursor {
  const unsigned char* p;
  size_t n, at = 0;
  size_t left() const { return n - at; }
  // the next line without its '\n' (at most 1024 bytes); false at the end or without a terminator
  bool line(std::string* out) {
    out->clear();
    while (at < n && out->size() <= 1024) {
      const char ch = (char)p[at++];
      if (ch == '\n') return true;
      out->push_back(ch);
    }
    return false;
  }
};

constexpr uint32_t kMaxSide = 65536;

// w * h * 3 floats, or null: the sides are 1..kMaxSide
float* alloc_rgb(uint32_t w, uint32_t h) { return static_cast<float*>(malloc((size_t)w * h * 3 * sizeof(float))); }

// (r, g, b, e) -> byte * 2^(e - 136), e = 0: black (the inverse of cvr_write_hdr's encoding up to
// its truncation; stb_image's convention)
void rgbe_to_float(const unsigned char* t, float* out) {
  if (t[3] == 0) {
    out[0] = out[1] = out[2] = 0.0f;
    return;
  }
  const float f = std::ldexp(1.0f, (int)t[3] - 136);
  out[0] = (float)t[0] * f;
  out[1] = (float)t[1] * f;
  out[2] = (float)t[2] * f;
}

int read_hdr(Cursor& c, uint32_t* w_out, uint32_t* h_out, float** rgb_out) {
  std::string ln;
  if (!c.line(&ln) || ln.compare(0, 2, "#?") != 0) return CVR_ERR_IO;
  bool format = false;
  for (;;) {
    if (!c.line(&ln)) return CVR_ERR_IO;
    if (ln.empty()) break;
    if (ln == "FORMAT=32-bit_rle_rgbe") format = true;
    else if (ln.compare(0, 7, "FORMAT=") == 0) return CVR_ERR_IO;
  }
  if (!format || !c.line(&ln)) return CVR_ERR_IO;
  unsigned long h = 0, w = 0;
  char tail = 0;
  if (sscanf(ln.c_str(), "-Y %lu +X %lu%c", &h, &w, &tail) != 2) return CVR_ERR_IO;
  if (w == 0 || h == 0 || w > kMaxSide || h > kMaxSide) return CVR_ERR_IO;
  // the fewest bytes a scanline can take: flat 4 w; run-length encoded a 4-byte marker and, per
  // channel, 2 bytes per run of up to 127 texels
  const bool can_rle = w >= 8 && w < 32768;
  const size_t min_line = can_rle ? std::min<size_t>(4 * w, 4 + 8 * ((w + 126) / 127)) : 4 * w;
  if (c.left() / min_line < h) return CVR_ERR_IO;
  float* rgb = alloc_rgb((uint32_t)w, (uint32_t)h);
  if (!rgb) return CVR_ERR_NOMEM;
  std::vector<unsigned char> line(4 * w);
  for (unsigned long y = 0; y < h; ++y) {
    bool ok = c.left() >= 4;
    if (ok && can_rle && c.p[c.at] == 2 && c.p[c.at + 1] == 2 && !(c.p[c.at + 2] & 0x80)) {
      ok = (((unsigned long)c.p[c.at + 2] << 8) | c.p[c.at + 3]) == w;
      c.at += 4;
      for (int ch = 0; ok && ch < 4; ++ch) {
        unsigned long x = 0;
        while (ok && x < w) {
          if (c.left() < 2) {
            ok = false;
            break;
          }
          unsigned count = c.p[c.at++];
          if (count > 128) {  // a run
            count -= 128;
            const unsigned char v = c.p[c.at++];
            if (count > w - x) {
              ok = false;
              break;
            }
            for (unsigned k = 0; k < count; ++k) line[4 * (x + k) + ch] = v;
          } else {  // literals
            if (count == 0 || count > w - x || c.left() < count) {
              ok = false;
              break;
            }
            for (unsigned k = 0; k < count; ++k) line[4 * (x + k) + ch] = c.p[c.at + k];
            c.at += count;
          }
          x += count;
        }
      }
    } else if (ok) {
      ok = c.left() >= 4 * w;
      if (ok) {
        memcpy(line.data(), c.p + c.at, 4 * w);
        c.at += 4 * w;
      }
    }
    if (!ok) {
      free(rgb);
      return CVR_ERR_IO;
    }
    for (unsigned long x = 0; x < w; ++x) rgbe_to_float(&line[4 * x], rgb + ((size_t)y * w + x) * 3);
  }
  *w_out = (uint32_t)w;
  *h_out = (uint32_t)h;
  *rgb_out = rgb;
  return CVR_OK;
}

// "PF\n<w> <h>\n<scale>\n", then h rows of w * 3 floats, the bottom row first; scale < 0: little
// endian; its magnitude multiplies every value
int read_pfm(Cursor& c, uint32_t* w_out, uint32_t* h_out, float** rgb_out) {
  // three whitespace-separated tokens after "PF", then exactly one whitespace byte
  c.at = 2;
  std::string tok[3];
  for (int i = 0; i < 3; ++i) {
    while (c.at < c.n && isspace(c.p[c.at])) ++c.at;
    while (c.at < c.n && !isspace(c.p[c.at]) && tok[i].size() < 64) tok[i].push_back((char)c.p[c.at++]);
    if (tok[i].empty() || tok[i].size() >= 64) return CVR_ERR_IO;
  }
  if (c.at >= c.n || !isspace(c.p[c.at])) return CVR_ERR_IO;
  ++c.at;
  char* end = nullptr;
  const unsigned long w = strtoul(tok[0].c_str(), &end, 10);
  if (*end || tok[0][0] == '-') return CVR_ERR_IO;
  const unsigned long h = strtoul(tok[1].c_str(), &end, 10);
  if (*end || tok[1][0] == '-') return CVR_ERR_IO;
  const double scale = strtod(tok[2].c_str(), &end);
  if (*end || !std::isfinite(scale) || scale == 0.0) return CVR_ERR_IO;
  if (w == 0 || h == 0 || w > kMaxSide || h > kMaxSide) return CVR_ERR_IO;
  if (c.left() / (12 * w) < h) return CVR_ERR_IO;
  float* rgb = alloc_rgb((uint32_t)w, (uint32_t)h);
  if (!rgb) return CVR_ERR_NOMEM;
  const bool little = scale < 0.0;
  const float mag = (float)std::fabs(scale);
  for (unsigned long y = 0; y < h; ++y) {
    const unsigned char* src = c.p + c.at + (size_t)(h - 1 - y) * w * 12;
    float* dst = rgb + (size_t)y * w * 3;
    for (size_t i = 0; i < (size_t)w * 3; ++i) {
      const unsigned char* b = src + 4 * i;
      const uint32_t bits = little ? (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24
                                   : (uint32_t)b[3] | (uint32_t)b[2] << 8 | (uint32_t)b[1] << 16 | (uint32_t)b[0] << 24;
      float v;
      memcpy(&v, &bits, 4);
      dst[i] = mag == 1.0f ? v : v * mag;
    }
  }
  *w_out = (uint32_t)w;
  *h_out = (uint32_t)h;
  *rgb_out = rgb;
  return CVR_OK;
}

}  // namespace

extern "C" {

int cvr_read_image(const char* path, uint32_t* width, uint32_t* height, float** rgb) {
  if (!path || !width || !height || !rgb) return CVR_ERR_INVALID;
  *width = *height = 0;
  *rgb = nullptr;
  FILE* fp = fopen(path, "rb");
  if (!fp) return CVR_ERR_IO;
  std::vector<unsigned char> bytes;
  unsigned char buf[65536];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), fp)) > 0) bytes.insert(bytes.end(), buf, buf + got);
  const bool bad = ferror(fp) != 0;
  fclose(fp);
  if (bad || bytes.size() < 3) return CVR_ERR_IO;
  Cursor c{bytes.data(), bytes.size()};
  if (bytes[0] == 'P' && bytes[1] == 'F' && isspace(bytes[2])) return read_pfm(c, width, height, rgb);
  if (bytes[0] == '#' && bytes[1] == '?') return read_hdr(c, width, height, rgb);
  return CVR_ERR_IO;
}

void cvr_free_image(float* rgb) { free(rgb); }

}  // extern "C"
