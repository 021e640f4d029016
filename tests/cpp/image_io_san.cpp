// cvr_read_image on the files named on the command line, for a build with the host sanitizers
// (tests/test_image_io.py compiles this file and csrc/cvr_image_io.cpp with
// g++ -fsanitize=address,undefined and runs it on its malformed and well-formed files).
// One line per file: "<status> <width> <height> <sum of the texels>"; a sanitizer report ends the
// program with a non-zero status.
#include <cstdio>

#include "cvr.h"

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    uint32_t w = 0, h = 0;
    float* rgb = nullptr;
    const int r = cvr_read_image(argv[i], &w, &h, &rgb);
    double sum = 0.0;
    if (r == CVR_OK)
      for (size_t k = 0; k < (size_t)w * h * 3; ++k) sum += rgb[k];  // touches every float the reader says it wrote
    std::printf("%d %u %u %.9g\n", r, w, h, sum);
    cvr_free_image(rgb);
  }
  return 0;
}
