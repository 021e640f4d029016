// cvr_main.cpp - command-line front end with the reference's flags
// (ConfigParser.cpp:10-165, Main.cpp:46-146), driving libcvr through its C
// ABI only.
//
//   cvr [--scene-file|-s] FILE [--scene-type Auto|MitsubaXml|Vdb|Raw|Mhd]
//       [--kernel|-k naiveSK|regenerationSK|...] [--algorithm|-a cudaVolPath]
//       [--iterations|-i N] [--resolution|-r W [H]] [--number-of-tiles X [Y]]
//       [--trials N] [--output|-o NAME] [--interactive BOOL]
//       [--use-unified-memory BOOL]
//   extensions: --synthetic bucky|manix|hetvol|cloud, --device N, --seed S,
//   --devices N|d0,d1,... (one context per device, each on its own host
//   thread: tile k -> device k mod N for --number-of-tiles, else 8x8-block
//   shards of the one tile; every device stores its pixels straight into one
//   pinned host image), --pfm (also write the float image as <output>.pfm),
//   --noise-target F [--min-iterations N] [--pass-iterations N] (an adaptive
//   render, cvr_render_adaptive: every 8x8 block is sampled until its relative
//   standard error is at most F, -i being the cap; also writes the samples map
//   as <output>_samples.hdr), --denoise [--denoise-sigma F] [--denoise-passes N] (also
//   write the variance-guided filter of the render, cvr_denoise, as <output>_denoised.hdr),
//   --features [--feature-step F] (also write the primary-ray feature buffers, cvr_features, as
//   <output>_albedo.hdr, <output>_alpha.hdr and <output>_depth.hdr), --denoise-guided
//   [--guide-sigma A Z O] (--denoise through the feature-guided filter, cvr_denoise_guided)
//   --preview FILE [--preview-light X Y Z] [--preview-shading A D S K] [--preview-knee F]
//   [--preview-background R G B] [--preview-unshaded] (also write the shaded emission-absorption
//   preview, cvr_preview, as FILE; with --iterations 0 without a render)
//   --preview-shadows F [--preview-shadow-res X Y Z] [--preview-shadow-step F] (the preview with
//   directional shadows of strength F from a light volume, cvr_build_light_volume and
//   cvr_preview_shadowed; needs --preview and --preview-light)
//   --field-stats, --histogram FILE [--histogram-bins N [M]], --gradient-range auto (the value range,
//   largest gradient magnitude and value-gradient histogram of a Raw scene's bytes, found on the
//   device: cvr_field_stats, cvr_field_histogram; with --iterations 0 without a render)
//   --project max|min|mean|iso FILE [--project-window LO HI] [--iso V] [--project-step F]
//   [--project-refine N] [--project-colour R G B] (also write a projection of a Raw scene's bytes,
//   cvr_field_project, as FILE: the maximum, minimum or mean along each camera ray shown through
//   the window LO..HI, or the first-hit isosurface at V lit by the field's gradient; the light,
//   the weights and the background are --preview-light, --preview-shading and
//   --preview-background; with --iterations 0 without a render)
//
// Differences from the reference, on purpose: the timer is wall clock (the
// reference uses clock(), i.e. CPU time, Main.cpp:51-77); main does not wait
// for Enter; --interactive true has no GL viewer here (out of scope, SURVEY
// §2.1) and falls back to the headless path with a notice.
#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "cvr.h"

namespace {

struct Options {
  std::string scene_file, scene_type = "Auto", algorithm = "cudaVolPath", kernel = "regenerationSK";
  std::string output, synthetic, rng_binding = "path", world_to_aabb = "reference", mk_compaction = "fixed";
  std::string devices;  // --devices: a count or a comma list of device ids
  std::string medium_format = "float";  // --medium-format
  std::string transfer_file, transfer_mode = "linear";  // --transfer, --transfer-mode
  std::string transfer2d_file;         // --transfer2d
  std::string transfer_labels_file, labels_file;  // --transfer-labels, --labels
  std::vector<float> gradient_range;   // --gradient-range GLO GHI
  bool gradient_auto = false;          // --gradient-range auto
  bool field_stats = false;            // --field-stats
  std::string histogram_file;          // --histogram FILE
  std::vector<unsigned> histogram_bins{256, 256};  // --histogram-bins N [M]
  std::vector<float> voxel_spacing{1.0f, 1.0f, 1.0f};  // --voxel-spacing X Y Z
  std::vector<unsigned> crop;          // --crop X0 Y0 Z0 X1 Y1 Z1
  std::vector<float> clip_planes;      // --clip-plane A B C D, four values per plane given
  std::string envmap;  // --envmap FILE
  float env_scale = 1.0f;
  double env_rotate_y = 0.0;  // degrees
  bool pfm = false;
  bool adaptive = false;  // --noise-target given
  float noise_target = 0.0f;
  unsigned min_iterations = 8, pass_iterations = 4;
  bool denoise = false;  // --denoise given
  float denoise_sigma = 4.0f;
  unsigned denoise_passes = 5;
  bool features = false;        // --features given
  float feature_step = 1.0f;
  std::string preview_file;     // --preview FILE
  std::vector<float> preview_light;  // --preview-light X Y Z (none: the headlight)
  float preview_shading[3] = {0.3f, 0.7f, 0.2f};  // --preview-shading A D S K: ambient, diffuse, specular ...
  unsigned preview_shininess_log2 = 4;            // ... and the exponent's log2
  float preview_knee = 0.05f;
  float preview_background[3] = {0.0f, 0.0f, 0.0f};
  bool preview_unshaded = false;
  float preview_shadows = 0.0f;              // --preview-shadows F: the strength ...
  bool preview_shadows_set = false;          // ... and whether it was given
  std::vector<unsigned> preview_shadow_res;  // --preview-shadow-res X Y Z (none: the default grid)
  float preview_shadow_step = 1.0f;          // --preview-shadow-step F: the light volume's march step
  std::string project_mode, project_file;  // --project max|min|mean|iso FILE
  std::vector<float> project_window;       // --project-window LO HI (none: 0 .. the largest byte)
  float project_iso = 0.0f;                // --iso V ...
  bool project_iso_set = false;            // ... (not given: half the largest byte)
  float project_step = 1.0f;
  unsigned project_refine = 4;
  float project_colour[3] = {1.0f, 1.0f, 1.0f};
  bool denoise_guided = false;  // --denoise-guided given
  float guide_sigma[3] = {0.4f, 0.1f, 0.4f};
  std::vector<float> default_albedo;
  bool interactive = true, unified = false;
  unsigned trials = 1, iterations = 20, device = 0, seed = 0;
  std::vector<unsigned> tiles{1, 1}, resolution{1024, 1024};
};

bool parse_bool(const std::string& v) { return v == "1" || v == "true" || v == "on" || v == "yes"; }

void usage() {
  printf(
      "Generic:\n"
      "  -h [ --help ]                      produce help message\n"
      "  -s [ --scene-file ] arg            scene file to parse\n"
      "  --scene-type arg (=Auto)           Auto, MitsubaXml, Vdb, Raw, Mhd (+ VdbSparse)\n"
      "  --interactive arg (=1)             (no GL viewer in this build: runs headless)\n"
      "  --trials arg (=1)                  number of times to run the algorithm\n"
      "  -a [ --algorithm ] arg (=cudaVolPath)\n"
      "  -k [ --kernel ] arg (=regenerationSK)\n"
      "  --number-of-tiles arg (=1 1)\n"
      "  --use-unified-memory arg (=0)      1: upload the grid as sparse 8^3 leaves\n"
      "Scene configuration override:\n"
      "  -i [ --iterations ] arg (=20)\n"
      "  -o [ --output ] arg\n"
      "  -r [ --resolution ] arg (=1024 1024)\n"
      "Extensions:\n"
      "  --synthetic bucky|manix|hetvol|cloud  use a built-in proxy scene\n"
      "  --device N, --seed S\n"
      "  --devices N|d0,d1,...              render on several devices at once (one context and host\n"
      "                                     thread each; ids may repeat): tile k -> device k mod N\n"
      "                                     with --number-of-tiles, else 8x8-block shards of the image;\n"
      "                                     one value is a count (pick one device with --device)\n"
      "  --medium-format float|half (=float)  storage precision of density, density cells and albedo on\n"
      "                                     the device: half rounds every voxel to IEEE binary16 and halves\n"
      "                                     their bytes (wave-pool scheduler; see CVR_OPT_MEDIUM_FORMAT)\n"
      "  --transfer FILE                    Raw scenes (and --synthetic bucky): classify the scene's bytes on\n"
      "                                     the device through the transfer function in FILE, 2..4096 lines\n"
      "                                     of 'r g b density' spanning byte 0 .. the largest byte, in place of\n"
      "                                     the reference's built-in table (cvr_set_medium_scalar)\n"
      "  --transfer-mode linear|ceil (=linear)  interpolate between table entries, or take entry ceil(x)\n"
      "  --transfer2d FILE                  Raw scenes (and --synthetic bucky): classify the scene's bytes by value\n"
      "                                     and gradient magnitude through the 2-D table in FILE: a first line\n"
      "                                     'n m', then n*m lines of 'r g b density', row by row (row j: gradient\n"
      "                                     entry j; n >= 2, m >= 2, n*m <= 4096), the columns spanning byte 0 ..\n"
      "                                     the largest byte (cvr_set_medium_gradient); needs --gradient-range,\n"
      "                                     excludes --transfer\n"
      "  --gradient-range GLO GHI           the gradient magnitudes the table's rows span (0 <= GLO < GHI)\n"
      "  --gradient-range auto              0 and the field's largest gradient magnitude, found on the device\n"
      "                                     (cvr_field_stats)\n"
      "  --voxel-spacing X Y Z (=1 1 1)     the voxel spacing the gradient is taken with (each > 0)\n"
      "  --field-stats                      Raw scenes (and --synthetic bucky): print the bytes' value range, largest\n"
      "                                     gradient magnitude and NaN counts (cvr_field_stats)\n"
      "  --histogram FILE                   Raw scenes (and --synthetic bucky): write the histogram of the bytes over\n"
      "                                     the nodes of an N x M table (cvr_field_histogram): a first line 'n m',\n"
      "                                     then m lines of n counts, row j the gradient bin j; the values span byte\n"
      "                                     0 .. the largest byte, the gradient --gradient-range (not needed with M 1)\n"
      "  --histogram-bins N [M] (=256 256)  value bins and gradient bins (N >= 2, N*M <= 65536; M omitted: 1, no gradient)\n"
      "                                     --field-stats, --histogram and --gradient-range auto take --voxel-spacing;\n"
      "                                     with --iterations 0 they run without a render\n"
      "  --transfer-labels FILE --labels FILE.raw\n"
      "                                     Raw scenes (and --synthetic bucky): classify the scene's bytes through one\n"
      "                                     table row per label (cvr_set_medium_scene_labels).  FILE is --transfer2d's\n"
      "                                     format, an 'n m' line and m*n lines 'r g b density' row by row, m >= 1 (row j\n"
      "                                     is label j's transfer function); FILE.raw holds one label byte per voxel.\n"
      "                                     --transfer-mode applies; excludes --transfer and --transfer2d; --field-stats\n"
      "                                     also prints the voxels per label\n"
      "  --crop X0 Y0 Z0 X1 Y1 Z1           with --transfer or --transfer2d: keep the voxels X0 <= x < X1, Y0 <= y < Y1,\n"
      "                                     Z0 <= z < Z1 (voxel indices; past the grid: to its end) and store the\n"
      "                                     others as empty (cvr_set_clip)\n"
      "  --clip-plane A B C D               with --transfer or --transfer2d, up to 8 times: keep the voxels with\n"
      "                                     A x + B y + C z + D >= 0 in voxel indices; --field-stats then also prints\n"
      "                                     the number of voxels the clip keeps, as the render's build counted\n"
      "                                     them (with --iterations 0 the medium is built once for the count)\n"
      "  --envmap FILE(.hdr|.pfm)           light the scene with a latitude-longitude environment map in place\n"
      "                                     of the constant white one (cvr_set_environment; every device's\n"
      "                                     context keeps a copy; not with naiveMK or --rng-binding thread)\n"
      "  --env-scale F (=1)                 multiply the map's radiance by F (finite, >= 0)\n"
      "  --env-rotate-y DEG (=0)            turn the map by DEG degrees about the +Y axis\n"
      "  --pfm                              also write the float image as <output>.pfm\n"
      "  --noise-target F                   adaptive render: sample every 8x8-pixel block until its relative\n"
      "                                     standard error (cvr_block_error, floor 0.01) is at most F, with\n"
      "                                     --iterations as the cap per block; prints the paths traced and\n"
      "                                     writes the samples map as <output>_samples.hdr (one device, one tile)\n"
      "  --min-iterations N (=8)            adaptive render: samples of every block before the first check\n"
      "  --pass-iterations N (=4)           adaptive render: samples added per pass (min and cap: multiples)\n"
      "  --denoise                          also write the render filtered by the variance-guided denoiser\n"
      "                                     (cvr_denoise, floor 0.01) as <output>_denoised.hdr (and .pfm with\n"
      "                                     --pfm); with --noise-target the adaptive session is filtered, else\n"
      "                                     the render runs as a session in which every block takes all\n"
      "                                     --iterations (>= 2) samples, two in the first launch and one per\n"
      "                                     later launch, which makes the output the same bits in every run\n"
      "                                     (one device, one tile)\n"
      "  --denoise-guided                   --denoise through the feature-guided filter (cvr_denoise_guided: the\n"
      "                                     feature pass guides the edge-stopping term); excludes --denoise\n"
      "  --guide-sigma A Z O (=0.4 0.1 0.4) guided filter: widths of the albedo, depth and opacity terms (<= 0: off)\n"
      "  --features                         also write the primary-ray feature buffers (cvr_features) as\n"
      "                                     <output>_albedo.hdr, <output>_alpha.hdr and <output>_depth.hdr (and\n"
      "                                     .pfm with --pfm); one tile on one device\n"
      "  --feature-step F (=1)              feature pass: march step in cells of the finest axis, 1/8..8\n"
      "  --preview FILE                     also write the shaded preview (cvr_preview: one deterministic ray\n"
      "                                     march per pixel, Blinn-Phong on the density gradient) as the\n"
      "                                     Radiance file FILE (and FILE.pfm with --pfm); takes --feature-step;\n"
      "                                     with --iterations 0 it runs without a render; one tile on one device\n"
      "  --preview-light X Y Z              preview: the direction towards the light (default: a headlight)\n"
      "  --preview-shading A D S K (=0.3 0.7 0.2 4)  preview: ambient, diffuse, specular, exponent 2^K (K 0..10)\n"
      "  --preview-knee F (=0.05)           preview: gradient magnitude of a half-lit sample, in majorants per cell\n"
      "  --preview-background R G B (=0 0 0)  preview: the colour behind the medium\n"
      "  --preview-unshaded                 preview: plain emission-absorption compositing, no light\n"
      "  --preview-shadows F                preview: directional shadows of strength F in [0, 1] from a light volume\n"
      "                                     (needs --preview and --preview-light)\n"
      "  --preview-shadow-res X Y Z         preview: the light volume's nodes (default: half the medium's, at most 256)\n"
      "  --preview-shadow-step F (=1)       preview: the step of the march towards the light, in cells\n"
      "  --project max|min|mean|iso FILE    Raw scenes (and --synthetic bucky): also write a projection of the bytes\n"
      "                                     (cvr_field_project): the maximum, minimum or mean along each camera ray, or\n"
      "                                     the first-hit isosurface lit by the field's gradient (--preview-light,\n"
      "                                     --preview-shading and --preview-background apply); with --iterations 0 it\n"
      "                                     runs without a render; one tile on one device\n"
      "  --project-window LO HI             projection: the values shown black and full colour (default: 0 and the\n"
      "                                     largest byte)\n"
      "  --iso V                            projection: the isosurface's level (default: half the largest byte)\n"
      "  --project-step F (=1)              projection: the march's step, in cells\n"
      "  --project-refine N (=4)            projection: bisections of the isosurface's bracket, 0..8\n"
      "  --project-colour R G B (=1 1 1)    projection: the full-scale colour, the surface's colour\n"
      "  --denoise-sigma F (=4)             denoiser: width of the edge-stopping term in standard deviations\n"
      "  --denoise-passes N (=5)            denoiser: a-trous passes, 1..6 (pass k has step 2^k)\n"
      "  --rng-binding path|thread (=path)  regenerationSK: thread = the reference's Rng(seed + tid)\n"
      "                                     per persistent thread (non-deterministic, SURVEY Q2)\n"
      "  --default-albedo r g b             VDB files without an albedo grid load with this albedo\n"
      "                                     (the reference refuses them, SURVEY Q17)\n"
      "  --world-to-aabb reference|fixed (=reference)  Woodcock density coordinate: the reference's\n"
      "                                     p - min/extent, or (p - min)/extent (SURVEY Q4)\n"
      "  --mk-compaction fixed|reference (=fixed)  naiveMK: keep every live path, or the reference's\n"
      "                                     end - begin - 1 (drops one per bounce, SURVEY Q11)\n");
}

bool is_flag(const char* a) { return a[0] == '-' && !(a[1] >= '0' && a[1] <= '9'); }

int parse(int argc, char** argv, Options& o) {
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    auto need = [&](const char* name) -> std::string {
      if (i + 1 >= argc) {
        fprintf(stderr, "[ConfigParser] Error: the required argument for option '%s' is missing\n", name);
        exit(2);
      }
      return argv[++i];
    };
    auto multi = [&](std::vector<unsigned>& dst) {
      dst.clear();
      while (i + 1 < argc && !is_flag(argv[i + 1])) dst.push_back((unsigned)strtoul(argv[++i], nullptr, 10));
      if (dst.empty()) {
        fprintf(stderr, "[ConfigParser] Error: option '%s' needs a value\n", a.c_str());
        exit(2);
      }
    };
    if (a == "-h" || a == "--help") return 1;
    else if (a == "-s" || a == "--scene-file") o.scene_file = need("scene-file");
    else if (a == "--scene-type") o.scene_type = need("scene-type");
    else if (a == "--interactive") o.interactive = parse_bool(need("interactive"));
    else if (a == "--trials") o.trials = (unsigned)strtoul(need("trials").c_str(), nullptr, 10);
    else if (a == "-a" || a == "--algorithm") o.algorithm = need("algorithm");
    else if (a == "-k" || a == "--kernel") o.kernel = need("kernel");
    else if (a == "--number-of-tiles") multi(o.tiles);
    else if (a == "--use-unified-memory") o.unified = parse_bool(need("use-unified-memory"));
    else if (a == "-i" || a == "--iterations") o.iterations = (unsigned)strtoul(need("iterations").c_str(), nullptr, 10);
    else if (a == "-o" || a == "--output") o.output = need("output");
    else if (a == "-r" || a == "--resolution") multi(o.resolution);
    else if (a == "--synthetic") o.synthetic = need("synthetic");
    else if (a == "--device") o.device = (unsigned)strtoul(need("device").c_str(), nullptr, 10);
    else if (a == "--devices") o.devices = need("devices");
    else if (a == "--medium-format") o.medium_format = need("medium-format");
    else if (a == "--transfer") o.transfer_file = need("transfer");
    else if (a == "--transfer-mode") o.transfer_mode = need("transfer-mode");
    else if (a == "--transfer2d") o.transfer2d_file = need("transfer2d");
    else if (a == "--transfer-labels") o.transfer_labels_file = need("transfer-labels");
    else if (a == "--labels") o.labels_file = need("labels");
    else if (a == "--gradient-range" || a == "--voxel-spacing") {
      const bool range = a == "--gradient-range";
      std::vector<float>& dst = range ? o.gradient_range : o.voxel_spacing;
      const size_t want = range ? 2 : 3;
      dst.clear();
      if (range && i + 1 < argc && std::string(argv[i + 1]) == "auto") {
        o.gradient_auto = true;
        ++i;
        continue;
      }
      o.gradient_auto = range ? false : o.gradient_auto;
      while (i + 1 < argc && dst.size() < want && !(argv[i + 1][0] == '-' && argv[i + 1][1] == '-'))
        dst.push_back(strtof(argv[++i], nullptr));
      if (dst.size() != want) {
        fprintf(stderr, "[ConfigParser] Error: %s needs %zu values\n", a.c_str(), want);
        return 2;
      }
    }
    else if (a == "--crop" || a == "--clip-plane") {
      // (a plane's coefficients may be negative: only another option ends the values; a crop's
      // are voxel indices, digits only, up to 2^32 - 1)
      const size_t want = a == "--crop" ? 6 : 4;
      size_t got = 0;
      if (a == "--crop") o.crop.clear();
      while (i + 1 < argc && got < want && !(argv[i + 1][0] == '-' && argv[i + 1][1] == '-')) {
        ++got;
        const char* v = argv[++i];
        char* end = nullptr;
        if (a == "--crop") {
          errno = 0;
          const unsigned long long u = strtoull(v, &end, 10);
          if (!(v[0] >= '0' && v[0] <= '9') || *end != '\0' || errno || u > 0xFFFFFFFFull) {
            fprintf(stderr, "[ConfigParser] Error: --crop value '%s' is not a voxel index (digits only, at most "
                            "4294967295)\n", v);
            return 2;
          }
          o.crop.push_back((unsigned)u);
        } else {
          const float f = strtof(v, &end);
          if (end == v || *end != '\0') {
            fprintf(stderr, "[ConfigParser] Error: --clip-plane value '%s' is not a number\n", v);
            return 2;
          }
          o.clip_planes.push_back(f);
        }
      }
      if (got != want) {
        fprintf(stderr, "[ConfigParser] Error: %s needs %zu values\n", a.c_str(), want);
        return 2;
      }
    }
    else if (a == "--field-stats") o.field_stats = true;
    else if (a == "--histogram") o.histogram_file = need("histogram");
    else if (a == "--histogram-bins") {
      o.histogram_bins.clear();
      while (i + 1 < argc && o.histogram_bins.size() < 2 && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9')
        o.histogram_bins.push_back((unsigned)strtoul(argv[++i], nullptr, 10));
      if (o.histogram_bins.size() == 1) o.histogram_bins.push_back(1u);
      if (o.histogram_bins.size() != 2) {
        fprintf(stderr, "[ConfigParser] Error: --histogram-bins needs 1 or 2 values\n");
        return 2;
      }
    }
    else if (a == "--envmap") o.envmap = need("envmap");
    else if (a == "--env-scale") o.env_scale = strtof(need("env-scale").c_str(), nullptr);
    else if (a == "--env-rotate-y") o.env_rotate_y = strtod(need("env-rotate-y").c_str(), nullptr);
    else if (a == "--pfm") o.pfm = true;
    else if (a == "--noise-target") {
      o.noise_target = strtof(need("noise-target").c_str(), nullptr);
      o.adaptive = true;
    }
    else if (a == "--min-iterations") o.min_iterations = (unsigned)strtoul(need("min-iterations").c_str(), nullptr, 10);
    else if (a == "--pass-iterations") o.pass_iterations = (unsigned)strtoul(need("pass-iterations").c_str(), nullptr, 10);
    else if (a == "--denoise") o.denoise = true;
    else if (a == "--denoise-guided") o.denoise_guided = true;
    else if (a == "--guide-sigma") {
      for (int k = 0; k < 3; ++k) o.guide_sigma[k] = strtof(need("guide-sigma").c_str(), nullptr);
    } else if (a == "--features") o.features = true;
    else if (a == "--preview") o.preview_file = need("preview");
    else if (a == "--preview-light") {
      o.preview_light.clear();
      for (int k = 0; k < 3; ++k) o.preview_light.push_back(strtof(need("preview-light").c_str(), nullptr));
    } else if (a == "--preview-shading") {
      for (int k = 0; k < 3; ++k) o.preview_shading[k] = strtof(need("preview-shading").c_str(), nullptr);
      o.preview_shininess_log2 = (unsigned)strtoul(need("preview-shading").c_str(), nullptr, 10);
    } else if (a == "--preview-knee") o.preview_knee = strtof(need("preview-knee").c_str(), nullptr);
    else if (a == "--preview-background") {
      for (int k = 0; k < 3; ++k) o.preview_background[k] = strtof(need("preview-background").c_str(), nullptr);
    } else if (a == "--preview-unshaded") o.preview_unshaded = true;
    else if (a == "--preview-shadows") {
      o.preview_shadows = strtof(need("preview-shadows").c_str(), nullptr);
      o.preview_shadows_set = true;
    } else if (a == "--preview-shadow-res") {
      o.preview_shadow_res.clear();
      for (int k = 0; k < 3; ++k) o.preview_shadow_res.push_back((unsigned)strtoul(need("preview-shadow-res").c_str(), nullptr, 10));
    } else if (a == "--preview-shadow-step") o.preview_shadow_step = strtof(need("preview-shadow-step").c_str(), nullptr);
    else if (a == "--project") {
      o.project_mode = need("project");
      o.project_file = need("project");
    } else if (a == "--project-window") {
      o.project_window.clear();
      for (int k = 0; k < 2; ++k) o.project_window.push_back(strtof(need("project-window").c_str(), nullptr));
    } else if (a == "--iso") {
      o.project_iso = strtof(need("iso").c_str(), nullptr);
      o.project_iso_set = true;
    } else if (a == "--project-step") o.project_step = strtof(need("project-step").c_str(), nullptr);
    else if (a == "--project-refine") o.project_refine = (unsigned)strtoul(need("project-refine").c_str(), nullptr, 10);
    else if (a == "--project-colour") {
      for (int k = 0; k < 3; ++k) o.project_colour[k] = strtof(need("project-colour").c_str(), nullptr);
    }
    else if (a == "--feature-step") o.feature_step = strtof(need("feature-step").c_str(), nullptr);
    else if (a == "--denoise-sigma") o.denoise_sigma = strtof(need("denoise-sigma").c_str(), nullptr);
    else if (a == "--denoise-passes") o.denoise_passes = (unsigned)strtoul(need("denoise-passes").c_str(), nullptr, 10);
    else if (a == "--rng-binding") o.rng_binding = need("rng-binding");
    else if (a == "--seed") o.seed = (unsigned)strtoul(need("seed").c_str(), nullptr, 10);
    else if (a == "--world-to-aabb") o.world_to_aabb = need("world-to-aabb");
    else if (a == "--mk-compaction") o.mk_compaction = need("mk-compaction");
    else if (a == "--default-albedo") {
      o.default_albedo.clear();
      while (i + 1 < argc && o.default_albedo.size() < 3 && !(argv[i + 1][0] == '-' && argv[i + 1][1] == '-'))
        o.default_albedo.push_back(strtof(argv[++i], nullptr));
      if (o.default_albedo.size() == 1) o.default_albedo.resize(3, o.default_albedo[0]);
      if (o.default_albedo.size() != 3) {
        fprintf(stderr, "[ConfigParser] Error: --default-albedo needs 1 or 3 values\n");
        return 2;
      }
    }
    else if (!is_flag(a.c_str()) && o.scene_file.empty()) o.scene_file = a;  // positional
    else {
      fprintf(stderr, "[ConfigParser] Error: unrecognised option '%s'\n", a.c_str());
      return 2;
    }
  }
  if (o.tiles.size() == 1) o.tiles.push_back(o.tiles[0]);
  if (o.resolution.size() == 1) o.resolution.push_back(o.resolution[0]);
  return 0;
}

// --devices: "N" (devices first..first+N-1; a single value is always a count: one
// device is chosen with --device) or "d0,d1,..." (two or more ids, which may repeat:
// several contexts on one device, each with its own stream and work queues).  An
// empty or non-numeric entry is an error (empty result).
bool parse_uint(const std::string& s, unsigned& v) {
  if (s.empty() || s.size() > 9) return false;
  for (char ch : s)
    if (ch < '0' || ch > '9') return false;
  v = (unsigned)strtoul(s.c_str(), nullptr, 10);
  return true;
}
std::vector<int> parse_devices(const std::string& v, unsigned first) {
  std::vector<int> d;
  if (v.empty()) return {(int)first};
  unsigned x = 0;
  if (v.find(',') == std::string::npos) {
    if (!parse_uint(v, x) || x == 0) return {};
    for (unsigned k = 0; k < x; ++k) d.push_back((int)(first + k));
    return d;
  }
  size_t p = 0;
  while (p <= v.size()) {
    const size_t q = std::min(v.find(',', p), v.size());
    if (!parse_uint(v.substr(p, q - p), x)) return {};
    d.push_back((int)x);
    p = q + 1;
  }
  return d;
}

// Portable float map (little-endian RGB, rows bottom to top): the image as floats,
// for comparisons the RGBE .hdr cannot hold.
int write_pfm(const std::string& path, const float* rgba, unsigned w, unsigned h) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return 1;
  fprintf(f, "PF\n%u %u\n-1.0\n", w, h);
  std::vector<float> row((size_t)w * 3);
  for (unsigned y = h; y-- > 0;) {
    for (unsigned x = 0; x < w; ++x)
      for (int c = 0; c < 3; ++c) row[(size_t)x * 3 + c] = rgba[((size_t)y * w + x) * 4 + c];
    fwrite(row.data(), sizeof(float), row.size(), f);
  }
  return fclose(f) != 0;
}

int scene_type_id(const std::string& t) {
  if (t == "Auto") return CVR_SCENE_AUTO;
  if (t == "MitsubaXml") return CVR_SCENE_MITSUBA_XML;
  if (t == "Vdb") return CVR_SCENE_VDB;
  if (t == "VdbSparse") return CVR_SCENE_VDB_SPARSE;
  if (t == "Raw") return CVR_SCENE_RAW;
  if (t == "Mhd") return CVR_SCENE_MHD;
  return -1;
}

// --transfer FILE: lines of 'r g b density' (blank lines and lines starting with # are skipped)
// into table; false with a message when the file cannot be read, a line does not hold four
// numbers, or there are not 2..4096 entries.
bool read_transfer(const std::string& path, std::vector<float>& table) {
  FILE* fp = fopen(path.c_str(), "r");
  if (!fp) {
    fprintf(stderr, "[ConfigParser] Error: --transfer: cannot read '%s'\n", path.c_str());
    return false;
  }
  char line[512];
  unsigned lineno = 0;
  bool ok = true;
  while (ok && fgets(line, sizeof(line), fp)) {
    ++lineno;
    const char* p = line;
    while (*p == ' ' || *p == '\t') ++p;
    if (*p == '#' || *p == '\n' || *p == '\r' || *p == 0) continue;
    float v[4];
    char extra;
    if (sscanf(p, "%f %f %f %f %c", &v[0], &v[1], &v[2], &v[3], &extra) != 4) {
      fprintf(stderr, "[ConfigParser] Error: --transfer: line %u of '%s' is not 'r g b density'\n", lineno, path.c_str());
      ok = false;
    }
    table.insert(table.end(), v, v + 4);
  }
  fclose(fp);
  if (ok && (table.size() < 8 || table.size() > 4 * 4096)) {
    fprintf(stderr, "[ConfigParser] Error: --transfer: '%s' holds %zu entries, a table has 2..4096\n", path.c_str(),
            table.size() / 4);
    ok = false;
  }
  return ok;
}

// the scene's grid resolution
struct Res3 {
  uint32_t v[3];
};
Res3 md_res_of(const cvr_scene* scene) {
  cvr_medium_desc md{};
  Res3 r{{0u, 0u, 0u}};
  if (cvr_scene_medium(scene, &md) == CVR_OK) memcpy(r.v, md.res, sizeof(r.v));
  return r;
}

// --field-stats, --gradient-range auto and --histogram: the scene's bytes as a u8 field with lo 0
// and hi the largest byte, on `device`.  The bytes are handed to the device calls in pinned,
// device-mapped host memory (this program links no HIP of its own); the context holds no medium.
// *gmax receives the largest gradient magnitude when the statistics ran.
int field_pass(const Options& o, int device, int kernel, const cvr_scene* scene, float* gmax) {
  const uint8_t* raw = nullptr;
  size_t n_raw = 0;
  cvr_medium_desc md{};
  if (cvr_scene_raw_bytes(scene, &raw, &n_raw) != CVR_OK || !n_raw || cvr_scene_medium(scene, &md) != CVR_OK ||
      n_raw != (size_t)md.res[0] * md.res[1] * md.res[2])
    return 1;
  void* pinned = nullptr;
  cvr_ctx* ctx = nullptr;
  auto done = [&](int code) {
    if (ctx) cvr_destroy(ctx);
    if (pinned) cvr_host_free(pinned);
    return code;
  };
  auto failed = [&]() {
    fprintf(stderr, "Error: %s\n", cvr_last_error(ctx));
    return done(1);
  };
  if (cvr_host_alloc(n_raw, &pinned) != CVR_OK || cvr_create(device, kernel, &ctx) != CVR_OK) return failed();
  memcpy(pinned, raw, n_raw);
  cvr_field_desc f{};
  memcpy(f.res, md.res, sizeof(f.res));
  f.scalar_type = CVR_SCALAR_U8;
  f.scalar = pinned;
  for (int k = 0; k < 3; ++k) f.spacing[k] = o.voxel_spacing[k];
  struct cvr_field_stats st {};
  if (o.field_stats || o.gradient_auto) {
    if (cvr_field_stats(ctx, &f, &st) != CVR_OK) return failed();
    *gmax = st.gmax;
    if (o.field_stats)
      printf("field statistics    : values %.9g .. %.9g, largest gradient magnitude %.9g, NaN values %llu, NaN "
             "gradients %llu\n",
             (double)st.vmin, (double)st.vmax, (double)st.gmax, (unsigned long long)st.nan_values,
             (unsigned long long)st.nan_gradients);
    if (o.gradient_auto && !(st.gmax > 0.0f && std::isfinite(st.gmax))) {
      fprintf(stderr, "[ConfigParser] Error: --gradient-range auto: the field's largest gradient magnitude is %g (a "
                      "constant field has no gradient range)\n", (double)st.gmax);
      return done(2);
    }
  }
  if (!o.histogram_file.empty()) {
    cvr_histogram_desc h{};
    h.n = o.histogram_bins[0], h.m = o.histogram_bins[1];
    h.lo = 0.0f, h.hi = (float)*std::max_element(raw, raw + n_raw);
    if (h.m > 1u) {
      h.glo = o.gradient_auto ? 0.0f : o.gradient_range[0];
      h.ghi = o.gradient_auto ? st.gmax : o.gradient_range[1];
    }
    std::vector<uint32_t> counts((size_t)h.n * h.m);
    if (cvr_field_histogram(ctx, &f, &h, counts.data()) != CVR_OK) return failed();
    FILE* fp = fopen(o.histogram_file.c_str(), "w");
    bool ok = fp != nullptr && fprintf(fp, "%u %u\n", h.n, h.m) > 0;
    for (uint32_t j = 0; ok && j < h.m; ++j)
      for (uint32_t i = 0; ok && i < h.n; ++i)
        ok = fprintf(fp, i + 1u < h.n ? "%u " : "%u\n", counts[(size_t)j * h.n + i]) > 0;
    if (fp && fclose(fp) != 0) ok = false;
    if (!ok) {
      fprintf(stderr, "Error: could not write %s\n", o.histogram_file.c_str());
      return done(1);
    }
    printf("histogram           : %u x %u bins over values %g .. %g", h.n, h.m, (double)h.lo, (double)h.hi);
    if (h.m > 1u) printf(" and gradient magnitudes %g .. %.9g", (double)h.glo, (double)h.ghi);
    printf(", written to %s\n", o.histogram_file.c_str());
  }
  return done(0);
}

// --project: the scene's bytes as a u8 field in the scene's box, handed to the device as field_pass
// hands them, projected for the camera into one W x H tile and written as o.project_file (and
// .pfm with --pfm).  The context holds no medium.
int project_pass(const Options& o, int device, int kernel, const cvr_scene* scene, const float inv_view[12],
                 const float r2v[2], const float full_res[2], unsigned W, unsigned H) {
  const uint8_t* raw = nullptr;
  size_t n_raw = 0;
  cvr_medium_desc md{};
  if (cvr_scene_raw_bytes(scene, &raw, &n_raw) != CVR_OK || !n_raw || cvr_scene_medium(scene, &md) != CVR_OK ||
      n_raw != (size_t)md.res[0] * md.res[1] * md.res[2])
    return 1;
  void* pinned = nullptr;
  cvr_ctx* ctx = nullptr;
  auto done = [&](int code) {
    if (ctx) cvr_destroy(ctx);
    if (pinned) cvr_host_free(pinned);
    return code;
  };
  auto failed = [&]() {
    fprintf(stderr, "Error: %s\n", cvr_last_error(ctx));
    return done(1);
  };
  if (cvr_host_alloc(n_raw, &pinned) != CVR_OK || cvr_create(device, kernel, &ctx) != CVR_OK) return failed();
  memcpy(pinned, raw, n_raw);
  cvr_field_desc f{};
  memcpy(f.res, md.res, sizeof(f.res));
  f.scalar_type = CVR_SCALAR_U8;
  f.scalar = pinned;
  const float top = (float)*std::max_element(raw, raw + n_raw);
  cvr_project_desc d{};
  d.mode = o.project_mode == "max" ? CVR_PROJECT_MAX : o.project_mode == "min" ? CVR_PROJECT_MIN
           : o.project_mode == "mean" ? CVR_PROJECT_MEAN : CVR_PROJECT_ISO;
  d.flags = o.preview_light.empty() ? CVR_PROJECT_HEADLIGHT : 0u;
  for (int k = 0; k < 3; ++k) {
    d.box_min[k] = md.box_min[k], d.box_max[k] = md.box_max[k];
    d.colour[k] = o.project_colour[k], d.background[k] = o.preview_background[k];
  }
  d.step = o.project_step, d.max_steps = 4096u;
  d.lo = o.project_window.empty() ? 0.0f : o.project_window[0];
  d.hi = o.project_window.empty() ? (top > 0.0f ? top : 1.0f) : o.project_window[1];
  d.iso = o.project_iso_set ? o.project_iso : 0.5f * top;
  d.refine = o.project_refine;
  for (size_t k = 0; k < o.preview_light.size(); ++k) d.light[k] = o.preview_light[k];
  d.ambient = o.preview_shading[0], d.diffuse = o.preview_shading[1], d.specular = o.preview_shading[2];
  d.shininess_log2 = o.preview_shininess_log2;
  std::vector<float> img((size_t)W * H * 4, 0.0f);
  if (cvr_set_camera(ctx, inv_view, r2v, full_res) != CVR_OK || cvr_set_resolution(ctx, W, H) != CVR_OK ||
      cvr_set_offset(ctx, 0, 0) != CVR_OK ||
      cvr_field_project(ctx, &f, &d, img.data(), nullptr, nullptr, img.size()) != CVR_OK)
    return failed();
  if (cvr_write_hdr(o.project_file.c_str(), img.data(), W, H) != CVR_OK ||
      (o.pfm && write_pfm(o.project_file + ".pfm", img.data(), W, H))) {
    fprintf(stderr, "Error: could not write %s%s\n", o.project_file.c_str(), o.pfm ? " / .pfm" : "");
    return done(1);
  }
  if (d.mode == CVR_PROJECT_ISO)
    printf("projection          : iso at %g, written to %s\n", (double)d.iso, o.project_file.c_str());
  else
    printf("projection          : %s over values %g .. %g, written to %s\n", o.project_mode.c_str(), (double)d.lo,
           (double)d.hi, o.project_file.c_str());
  return done(0);
}

// --transfer2d FILE: a first data line 'n m', then n * m lines of 'r g b density', row by row
// (blank lines and lines starting with # are skipped) into table; false with a message when the
// file cannot be read, a line is not what it should be, or the entries are not n * m.
// (--transfer-labels reads the same format with m >= 1: opt names the option, min_m its smallest m)
bool read_transfer2d(const std::string& path, std::vector<float>& table, unsigned& n, unsigned& m,
                     const char* opt = "--transfer2d", unsigned min_m = 2) {
  FILE* fp = fopen(path.c_str(), "r");
  if (!fp) {
    fprintf(stderr, "[ConfigParser] Error: %s: cannot read '%s'\n", opt, path.c_str());
    return false;
  }
  char line[512];
  unsigned lineno = 0;
  bool ok = true, have_size = false;
  n = m = 0;
  while (ok && fgets(line, sizeof(line), fp)) {
    ++lineno;
    const char* p = line;
    while (*p == ' ' || *p == '\t') ++p;
    if (*p == '#' || *p == '\n' || *p == '\r' || *p == 0) continue;
    char extra;
    if (!have_size) {
      if (sscanf(p, "%u %u %c", &n, &m, &extra) != 2) {
        fprintf(stderr, "[ConfigParser] Error: %s: line %u of '%s' is not 'n m'\n", opt, lineno, path.c_str());
        ok = false;
      } else if (n < 2 || m < min_m || (unsigned long long)n * m > 4096 || (min_m < 2 && m > 256)) {
        fprintf(stderr, "[ConfigParser] Error: %s: '%s' declares a %u x %u table: n >= 2, m >= %u%s, n*m <= 4096\n", opt,
                path.c_str(), n, m, min_m, min_m < 2 ? " and <= 256" : "");
        ok = false;
      }
      have_size = true;
      continue;
    }
    float v[4];
    if (sscanf(p, "%f %f %f %f %c", &v[0], &v[1], &v[2], &v[3], &extra) != 4) {
      fprintf(stderr, "[ConfigParser] Error: %s: line %u of '%s' is not 'r g b density'\n", opt, lineno,
              path.c_str());
      ok = false;
    }
    table.insert(table.end(), v, v + 4);
    if (ok && table.size() > (size_t)4 * n * m) break;  // (too many: counted below)
  }
  fclose(fp);
  if (ok && !have_size) {
    fprintf(stderr, "[ConfigParser] Error: %s: '%s' holds no 'n m' line\n", opt, path.c_str());
    ok = false;
  }
  if (ok && table.size() != (size_t)4 * n * m) {
    fprintf(stderr, "[ConfigParser] Error: %s: '%s' holds %s %u x %u = %u entries\n", opt, path.c_str(),
            table.size() < (size_t)4 * n * m ? "fewer than its" : "more than its", n, m, n * m);
    ok = false;
  }
  return ok;
}

}  // namespace

int main(int argc, char** argv) {
  Options o;
  int pr = parse(argc, argv, o);
  if (pr == 1) {
    usage();
    return 0;
  }
  if (pr) return pr;
  if (o.algorithm != "cudaVolPath") {
    fprintf(stderr, "[ConfigParser] algorithm %s not present in the list of algorithms\n", o.algorithm.c_str());
    return 2;
  }
  const int kernel = cvr_kernel_from_name(o.kernel.c_str());
  if (kernel == CVR_KERNEL_UNKNOWN) {  // RendererFactory.h:75-76 throws
    fprintf(stderr, "[RendererFactory] Error: kernel %s unknown\n", o.kernel.c_str());
    return 2;
  }
  if ((o.preview_shadows_set || !o.preview_shadow_res.empty()) &&
      (!o.preview_shadows_set || o.preview_file.empty() || o.preview_light.empty())) {
    fprintf(stderr, "[ConfigParser] Error: %s\n",
            !o.preview_shadows_set ? "--preview-shadow-res needs --preview-shadows F"
                                   : "--preview-shadows needs --preview FILE and --preview-light X Y Z (the shadows' "
                                     "directional light)");
    return 2;
  }
  cvr_scene* scene = nullptr;
  int r;
  if (!o.synthetic.empty()) {
    r = cvr_scene_synthetic(o.synthetic.c_str(), o.seed, nullptr, &scene);
  } else {
    if (o.scene_file.empty()) {
      fprintf(stderr, "Error: no scene file provided\n");
      return 2;
    }
    const int st = scene_type_id(o.scene_type);
    if (st < 0) {
      fprintf(stderr, "Error: scene type not correct\n");
      return 2;
    }
    cvr_load_options lo{};
    if (!o.default_albedo.empty()) {
      lo.flags = CVR_LOAD_DEFAULT_ALBEDO;
      for (int k = 0; k < 3; ++k) lo.default_albedo[k] = o.default_albedo[k];
    }
    r = cvr_scene_load_ex(o.scene_file.c_str(), st, &lo, &scene);
  }
  if (r != CVR_OK) {
    fprintf(stderr, "Error: could not load scene (%d): %s\n", r, cvr_last_error(nullptr));
    return 1;
  }
  if (!o.transfer2d_file.empty() && !o.transfer_file.empty()) {
    fprintf(stderr, "[ConfigParser] Error: --transfer2d excludes --transfer\n");
    return 2;
  }
  if (!o.transfer_labels_file.empty() && (!o.transfer_file.empty() || !o.transfer2d_file.empty())) {
    fprintf(stderr, "[ConfigParser] Error: --transfer-labels excludes --transfer and --transfer2d\n");
    return 2;
  }
  if (o.transfer_labels_file.empty() != o.labels_file.empty()) {
    fprintf(stderr, "[ConfigParser] Error: --transfer-labels FILE and --labels FILE.raw go together\n");
    return 2;
  }
  // --transfer: the table, and a scene that has one byte per voxel to classify
  std::vector<float> transfer_table;
  cvr_transfer_desc transfer{};
  if (o.transfer_mode != "linear" && o.transfer_mode != "ceil") {
    fprintf(stderr, "[ConfigParser] Error: --transfer-mode must be linear or ceil\n");
    return 2;
  }
  if (!o.transfer_file.empty()) {
    const uint8_t* raw = nullptr;
    size_t n_raw = 0;
    if (cvr_scene_raw_bytes(scene, &raw, &n_raw) != CVR_OK || !n_raw) {
      fprintf(stderr, "[ConfigParser] Error: --transfer applies to Raw scenes only (and --synthetic bucky): this "
                      "scene has no scalar bytes to classify\n");
      return 2;
    }
    if (!read_transfer(o.transfer_file, transfer_table)) return 2;
    transfer.n = (uint32_t)(transfer_table.size() / 4);
    transfer.flags = o.transfer_mode == "ceil" ? CVR_TF_CEIL : 0;
    transfer.table = transfer_table.data();
  }
  // --transfer2d: the 2-D table, its gradient range and the voxel spacing
  std::vector<float> transfer2d_table;
  cvr_gradient_transfer_desc transfer2d{};
  const bool want_histogram = !o.histogram_file.empty(), histogram_2d = want_histogram && o.histogram_bins[1] > 1u;
  const bool field_work = o.field_stats || want_histogram || o.gradient_auto;
  if (o.transfer2d_file.empty() && !want_histogram && (!o.gradient_range.empty() || o.gradient_auto)) {
    fprintf(stderr, "[ConfigParser] Error: --gradient-range applies to --transfer2d only (and to --histogram)\n");
    return 2;
  }
  const bool project = !o.project_file.empty();
  if (project && o.project_mode != "max" && o.project_mode != "min" && o.project_mode != "mean" && o.project_mode != "iso") {
    fprintf(stderr, "[ConfigParser] Error: --project takes max, min, mean or iso and a file name\n");
    return 2;
  }
  if (field_work || project) {
    const uint8_t* raw = nullptr;
    size_t n_raw = 0;
    if (cvr_scene_raw_bytes(scene, &raw, &n_raw) != CVR_OK || !n_raw) {
      fprintf(stderr, "[ConfigParser] Error: %s applies to Raw scenes only (and --synthetic bucky): this scene has no "
                      "scalar bytes\n", o.field_stats ? "--field-stats" : want_histogram ? "--histogram"
                                        : o.gradient_auto ? "--gradient-range auto" : "--project");
      return 2;
    }
  }
  if (field_work) {
    const unsigned hn = o.histogram_bins[0], hm = o.histogram_bins[1];
    if (want_histogram && (hn < 2u || hm < 1u || (unsigned long long)hn * hm > 65536ull)) {
      fprintf(stderr, "[ConfigParser] Error: --histogram-bins %u %u: N >= 2, M >= 1, N*M <= 65536\n", hn, hm);
      return 2;
    }
    if (histogram_2d && !o.gradient_auto && o.gradient_range.size() != 2) {
      fprintf(stderr, "[ConfigParser] Error: --histogram with M > 1 needs --gradient-range GLO GHI (or auto)\n");
      return 2;
    }
    if (histogram_2d && !o.gradient_auto) {
      const float glo = o.gradient_range[0], ghi = o.gradient_range[1];
      if (!std::isfinite(glo) || !std::isfinite(ghi) || !(glo >= 0.0f) || !(ghi > glo)) {
        fprintf(stderr, "[ConfigParser] Error: --gradient-range must be finite with 0 <= GLO < GHI\n");
        return 2;
      }
    }
    for (float v : o.voxel_spacing)
      if (!std::isfinite(v) || !(v > 0.0f)) {
        fprintf(stderr, "[ConfigParser] Error: --voxel-spacing must be three finite values > 0\n");
        return 2;
      }
  } else if (o.histogram_bins != std::vector<unsigned>{256u, 256u}) {
    fprintf(stderr, "[ConfigParser] Error: --histogram-bins applies to --histogram only\n");
    return 2;
  }
  if (!o.transfer2d_file.empty()) {
    const uint8_t* raw = nullptr;
    size_t n_raw = 0;
    if (cvr_scene_raw_bytes(scene, &raw, &n_raw) != CVR_OK || !n_raw) {
      fprintf(stderr, "[ConfigParser] Error: --transfer2d applies to Raw scenes only (and --synthetic bucky): this "
                      "scene has no scalar bytes to classify\n");
      return 2;
    }
    if (o.gradient_range.size() != 2 && !o.gradient_auto) {
      fprintf(stderr, "[ConfigParser] Error: --transfer2d needs --gradient-range GLO GHI\n");
      return 2;
    }
    // (auto: a placeholder range here, the device statistics' below)
    const float glo = o.gradient_auto ? 0.0f : o.gradient_range[0], ghi = o.gradient_auto ? 1.0f : o.gradient_range[1];
    if (!std::isfinite(glo) || !std::isfinite(ghi) || !(glo >= 0.0f) || !(ghi > glo)) {
      fprintf(stderr, "[ConfigParser] Error: --gradient-range must be finite with 0 <= GLO < GHI\n");
      return 2;
    }
    for (float v : o.voxel_spacing)
      if (!std::isfinite(v) || !(v > 0.0f)) {
        fprintf(stderr, "[ConfigParser] Error: --voxel-spacing must be three finite values > 0\n");
        return 2;
      }
    if (!read_transfer2d(o.transfer2d_file, transfer2d_table, transfer2d.n, transfer2d.m)) return 2;
    transfer2d.table = transfer2d_table.data();
    transfer2d.glo = glo;
    transfer2d.ghi = ghi;
    for (int k = 0; k < 3; ++k) transfer2d.spacing[k] = o.voxel_spacing[k];
  }
  // --transfer-labels, --labels: one table row per label byte, and the label volume
  std::vector<float> label_table;
  std::vector<uint8_t> label_bytes;
  cvr_label_transfer_desc transfer_labels{};
  if (!o.transfer_labels_file.empty()) {
    const uint8_t* raw = nullptr;
    size_t n_raw = 0;
    if (cvr_scene_raw_bytes(scene, &raw, &n_raw) != CVR_OK || !n_raw) {
      fprintf(stderr, "[ConfigParser] Error: --transfer-labels applies to Raw scenes only (and --synthetic bucky): this "
                      "scene has no scalar bytes to classify\n");
      return 2;
    }
    if (!read_transfer2d(o.transfer_labels_file, label_table, transfer_labels.n, transfer_labels.m, "--transfer-labels", 1))
      return 2;
    transfer_labels.flags = o.transfer_mode == "ceil" ? CVR_TF_CEIL : 0;
    transfer_labels.table = label_table.data();
    FILE* fp = fopen(o.labels_file.c_str(), "rb");
    if (!fp) {
      fprintf(stderr, "[ConfigParser] Error: --labels: cannot read '%s'\n", o.labels_file.c_str());
      return 2;
    }
    label_bytes.resize(n_raw + 1);  // (one more: a longer file shows)
    const size_t got = fread(label_bytes.data(), 1, n_raw + 1, fp);
    fclose(fp);
    if (got != n_raw) {
      fprintf(stderr, "[ConfigParser] Error: --labels: '%s' holds %s %zu bytes, one per voxel of the scene\n",
              o.labels_file.c_str(), got < n_raw ? "fewer than the" : "more than the", n_raw);
      return 2;
    }
    label_bytes.resize(n_raw);
  }
  // --crop, --clip-plane: the clip region of the device build (the host uploads do not clip)
  cvr_clip_desc clip{};
  const bool have_clip = !o.crop.empty() || !o.clip_planes.empty();
  if (have_clip) {
    const uint8_t* raw = nullptr;
    size_t n_raw = 0;
    if (cvr_scene_raw_bytes(scene, &raw, &n_raw) != CVR_OK || !n_raw) {
      fprintf(stderr, "[ConfigParser] Error: --crop and --clip-plane apply to Raw scenes only (and --synthetic bucky): "
                      "this scene has no scalar bytes to classify on the device\n");
      return 2;
    }
    if (!transfer.n && !transfer2d.n && !transfer_labels.n) {
      fprintf(stderr, "[ConfigParser] Error: --crop and --clip-plane need --transfer or --transfer2d (or --transfer-labels; the clip is applied "
                      "where the device build classifies the voxel)\n");
      return 2;
    }
    if (o.clip_planes.size() > 4u * CVR_CLIP_MAX_PLANES) {
      fprintf(stderr, "[ConfigParser] Error: at most %d --clip-plane\n", CVR_CLIP_MAX_PLANES);
      return 2;
    }
    for (int k = 0; k < 3; ++k) {
      clip.lo[k] = o.crop.empty() ? 0u : o.crop[k];
      clip.hi[k] = o.crop.empty() ? 0xFFFFFFFFu : o.crop[3 + k];
    }
    clip.n_planes = (uint32_t)(o.clip_planes.size() / 4);
    memcpy(clip.planes, o.clip_planes.data(), o.clip_planes.size() * sizeof(float));
    // (the library's own check of the descriptor, before any device is touched)
    const Res3 clip_res = md_res_of(scene);
    if (cvr_clip_host(clip_res.v, &clip, nullptr, nullptr, nullptr) != CVR_OK) {
      fprintf(stderr, "[ConfigParser] Error: --crop / --clip-plane: %s\n", cvr_last_error(nullptr));
      return 2;
    }
  }
  // --envmap: the file's texels and the descriptor every context takes its copy from
  float* env_rgb = nullptr;
  cvr_environment_desc env{};
  if (!o.envmap.empty()) {
    if ((r = cvr_read_image(o.envmap.c_str(), &env.width, &env.height, &env_rgb)) != CVR_OK) {
      fprintf(stderr, "[ConfigParser] Error: --envmap: cannot read '%s' as a Radiance .hdr or a colour .pfm (%d)\n",
              o.envmap.c_str(), r);
      return 2;
    }
    env.channels = 3;
    env.location = CVR_ENV_HOST;
    env.pixels = env_rgb;
    env.scale = o.env_scale;
    if (o.env_rotate_y != 0.0) {  // world-to-environment: the map turns by +DEG about +Y
      const double a = o.env_rotate_y * (3.14159265358979323846 / 180.0);
      const float cs = (float)std::cos(a), sn = (float)std::sin(a);
      const float R[9] = {cs, 0.0f, -sn, 0.0f, 1.0f, 0.0f, sn, 0.0f, cs};
      memcpy(env.rotation, R, sizeof(R));
    }
    printf("[ConfigParser] environment map %s: %ux%u, scale %g, rotated %g degrees about +Y.\n", o.envmap.c_str(),
           env.width, env.height, (double)env.scale, o.env_rotate_y);
  }
  printf("[ConfigParser] kernel set to %s.\n[ConfigParser] iterations set to %u.\n", o.kernel.c_str(), o.iterations);
  if (o.interactive) printf("[ConfigParser] interactive viewer not available in this build; rendering headless.\n");
  if (o.output.empty())  // Config::operator<< (Config.h:237-248)
    o.output = "algorithm_" + o.algorithm + "_kernel_" + o.kernel + "_iter_" + std::to_string(o.iterations);

  // Medium upload: dense textures as the reference; the 8^3-leaf upload for
  // sparse-only scenes, for --use-unified-memory true (the reference's
  // HostDeviceMedium choice for scenes too big for device memory,
  // Config.h:147-156), and when the dense grid is rejected as too large.
  cvr_medium_desc md;
  cvr_sparse_medium_desc sd;
  bool sparse = cvr_scene_is_sparse(scene) || o.unified;
  if (!sparse) cvr_scene_medium(scene, &md);
  if (sparse && (r = cvr_scene_sparse_medium(scene, &sd)) != CVR_OK) {
    fprintf(stderr, "Error: sparse view of the scene failed (%d)\n", r);
    return 1;
  }
  const unsigned W = o.resolution[0], H = o.resolution[1];
  float inv_view[12], r2v[2];
  cvr_scene_camera(scene, W, H, inv_view, r2v);  // default camera; XML scenes carry their fov
  const float full_res[2] = {(float)W, (float)H};
  std::vector<float> image((size_t)W * H * 4, 0.0f);
  std::vector<double> times;
  double mean = 0;
  if (o.rng_binding != "path" && o.rng_binding != "thread") {
    fprintf(stderr, "[ConfigParser] Error: --rng-binding must be path or thread\n");
    return 2;
  }
  if (o.world_to_aabb != "reference" && o.world_to_aabb != "fixed") {
    fprintf(stderr, "[ConfigParser] Error: --world-to-aabb must be reference or fixed\n");
    return 2;
  }
  if (o.mk_compaction != "fixed" && o.mk_compaction != "reference") {
    fprintf(stderr, "[ConfigParser] Error: --mk-compaction must be fixed or reference\n");
    return 2;
  }
  if (o.medium_format != "float" && o.medium_format != "half") {
    fprintf(stderr, "[ConfigParser] Error: --medium-format must be float or half\n");
    return 2;
  }
  // One context: its options, the medium (its own upload, or `share`'s device copy when
  // another context on the same device already holds it), the camera.
  auto make_ctx = [&](int device, cvr_ctx* share) -> cvr_ctx* {
    cvr_ctx* ctx = nullptr;
    if (cvr_create(device, kernel, &ctx) != CVR_OK) {
      fprintf(stderr, "Error: %s\n", cvr_last_error(nullptr));
      return nullptr;
    }
    int rc = cvr_set_seed(ctx, o.seed);
    if (!rc && o.rng_binding == "thread") rc = cvr_set_option(ctx, CVR_OPT_RNG_BINDING, 1);
    if (!rc && o.world_to_aabb == "fixed") rc = cvr_set_option(ctx, CVR_OPT_WORLD_TO_AABB, 1);
    if (!rc && o.mk_compaction == "reference") rc = cvr_set_option(ctx, CVR_OPT_MK_COMPACTION, 1);
    if (!rc && o.medium_format == "half") rc = cvr_set_option(ctx, CVR_OPT_MEDIUM_FORMAT, CVR_FORMAT_F16);
    if (!rc && have_clip && !share) rc = cvr_set_clip(ctx, &clip);
    if (!rc && share) {
      rc = cvr_share_medium(ctx, share);
    } else if (!rc && transfer2d.n) {
      rc = cvr_set_medium_scene_gradient(ctx, scene, &transfer2d, sparse ? CVR_DEVMED_SPARSE : 0);
    } else if (!rc && transfer_labels.n) {
      rc = cvr_set_medium_scene_labels(ctx, scene, &transfer_labels, label_bytes.data(), label_bytes.size(),
                                       sparse ? CVR_DEVMED_SPARSE : 0);
    } else if (!rc && transfer.n) {
      rc = cvr_set_medium_scene_transfer(ctx, scene, &transfer, sparse ? CVR_DEVMED_SPARSE : 0);
    } else if (!rc) {
      if (!sparse && (rc = cvr_set_medium(ctx, &md)) == CVR_ERR_UNSUPPORTED) {
        printf("[Scene] dense grid rejected (%s); using the sparse leaf upload\n", cvr_last_error(ctx));
        if ((rc = cvr_scene_sparse_medium(scene, &sd)) == CVR_OK) sparse = true;
      }
      if (!rc && sparse) rc = cvr_set_medium_sparse(ctx, &sd);
    }
    if (!rc) rc = cvr_set_camera(ctx, inv_view, r2v, full_res);
    if (!rc && env_rgb) rc = cvr_set_environment(ctx, &env);
    if (!rc) rc = cvr_init(ctx);
    if (rc) {
      fprintf(stderr, "Error: %s\n", cvr_last_error(ctx));
      cvr_destroy(ctx);
      return nullptr;
    }
    return ctx;
  };
  // --field-stats with a clip: the kept voxels, as the build of ctx's medium counted them
  auto print_kept = [&](cvr_ctx* ctx) -> int {
    uint64_t kept = 0;
    if (cvr_medium_clip_info(ctx, nullptr, &kept) != CVR_OK) {
      fprintf(stderr, "Error: %s\n", cvr_last_error(ctx));
      return 1;
    }
    const Res3 res = md_res_of(scene);
    printf("clip                : kept voxels %llu of %llu\n", (unsigned long long)kept,
           (unsigned long long)res.v[0] * res.v[1] * res.v[2]);
    return 0;
  };
  // --field-stats with --transfer-labels: the kept voxels per label byte, as the build counted them
  auto print_labels = [&](cvr_ctx* ctx) -> int {
    uint32_t rows = 0;
    uint64_t counts[256];
    if (cvr_medium_label_info(ctx, &rows, counts) != CVR_OK) {
      fprintf(stderr, "Error: %s\n", cvr_last_error(ctx));
      return 1;
    }
    printf("labels              : %u table rows; kept voxels per label byte:\n", rows);
    for (unsigned b = 0; b < 256; ++b)
      if (counts[b]) printf("  label %u: %llu\n", b, (unsigned long long)counts[b]);
    return 0;
  };
  const bool have_labels = transfer_labels.n != 0;
  const std::vector<int> devs = parse_devices(o.devices, o.device);
  if (devs.empty()) {
    fprintf(stderr, "[ConfigParser] Error: --devices needs a count (N >= 1) or a list of two or more device ids "
                    "(d0,d1,...), digits only\n");
    return 2;
  }
  if (field_work) {
    float gmax = 0.0f;
    if (int fr = field_pass(o, devs[0], kernel, scene, &gmax)) return fr;
    if (o.gradient_auto && transfer2d.n) {
      transfer2d.glo = 0.0f;
      transfer2d.ghi = gmax;
      printf("[ConfigParser] gradient range set to 0 .. %.9g.\n", (double)gmax);
    }
    if (o.iterations == 0) {  // the field's numbers alone: no render, no image
      if (o.field_stats && (have_clip || have_labels)) {
        // the kept voxels are counted by the build itself, and nothing renders: a context of this
        // pass's own builds the medium once for the count
        cvr_ctx* c = make_ctx(devs[0], nullptr);
        if (!c) return 1;
        int kr = have_clip ? print_kept(c) : 0;
        if (!kr && have_labels) kr = print_labels(c);
        cvr_destroy(c);
        if (kr) return kr;
      }
      if (o.preview_file.empty() && !project) {
        cvr_free_image(env_rgb);
        return 0;
      }
    }
  }
  const unsigned ntiles = o.tiles[0] * o.tiles[1];
  size_t n_dev = devs.size();
  if (o.denoise && o.denoise_guided) {
    fprintf(stderr, "[ConfigParser] Error: --denoise-guided excludes --denoise (one filtered image)\n");
    return 2;
  }
  const bool filtered = o.denoise || o.denoise_guided;
  const bool preview = !o.preview_file.empty();
  if ((o.adaptive || filtered || o.features || preview || project) && (n_dev > 1 || ntiles > 1)) {
    fprintf(stderr, "[ConfigParser] Error: %s renders one tile on one device (no --devices > 1, no "
                    "--number-of-tiles above 1 1)\n",
            o.adaptive ? "--noise-target" : o.denoise ? "--denoise" : o.denoise_guided ? "--denoise-guided"
                                                                : o.features     ? "--features"
                                                                : preview        ? "--preview"
                                                                                 : "--project");
    return 2;
  }
  // --preview: the pass on ctx's medium and camera, written as FILE (and FILE.pfm with --pfm)
  auto write_preview = [&](cvr_ctx* ctx) -> int {
    cvr_preview_desc pd{};
    pd.march = {o.feature_step, 1.0f / 256.0f, 4096u, 0u};
    pd.ambient = o.preview_shading[0], pd.diffuse = o.preview_shading[1], pd.specular = o.preview_shading[2];
    pd.shininess_log2 = o.preview_shininess_log2;
    pd.knee = o.preview_knee;
    for (int k = 0; k < 3; ++k) pd.background[k] = o.preview_background[k];
    for (size_t k = 0; k < o.preview_light.size(); ++k) pd.light[k] = o.preview_light[k];
    pd.flags = (o.preview_unshaded ? CVR_PREVIEW_UNSHADED : 0u) | (o.preview_light.empty() ? CVR_PREVIEW_HEADLIGHT : 0u);
    std::vector<float> img((size_t)W * H * 4, 0.0f);
    int rc = cvr_set_resolution(ctx, W, H);
    if (!rc) rc = cvr_set_offset(ctx, 0, 0);
    if (!rc && o.preview_shadows_set) {
      cvr_light_volume_desc vd{};
      for (int k = 0; k < 3; ++k) vd.light[k] = o.preview_light[k];
      vd.march = {o.preview_shadow_step, 1.0f / 256.0f, 4096u, 0u};
      if (o.preview_shadow_res.empty()) rc = cvr_light_volume_default_res(ctx, vd.res);
      for (size_t k = 0; k < o.preview_shadow_res.size(); ++k) vd.res[k] = o.preview_shadow_res[k];
      if (!rc) rc = cvr_build_light_volume(ctx, &vd);
      if (!rc) rc = cvr_preview_shadowed(ctx, &pd, o.preview_shadows, img.data(), img.size());
    } else if (!rc) {
      rc = cvr_preview(ctx, &pd, img.data(), img.size());
    }
    if (rc != CVR_OK) {
      fprintf(stderr, "Error: %s\n", cvr_last_error(ctx));
      return 1;
    }
    if (cvr_write_hdr(o.preview_file.c_str(), img.data(), W, H) != CVR_OK ||
        (o.pfm && write_pfm(o.preview_file + ".pfm", img.data(), W, H))) {
      fprintf(stderr, "Error: could not write %s%s\n", o.preview_file.c_str(), o.pfm ? " / .pfm" : "");
      return 1;
    }
    printf("preview             : %s\n", o.preview_file.c_str());
    return 0;
  };
  if (project) {  // the projection needs no medium: a context of its own, before any render
    if (int pr = project_pass(o, devs[0], kernel, scene, inv_view, r2v, full_res, W, H)) return pr;
    if (o.iterations == 0 && !preview) {
      cvr_free_image(env_rgb);
      cvr_scene_destroy(scene);
      return 0;
    }
  }
  if (preview && o.iterations == 0) {  // the preview alone: no render, no image
    cvr_ctx* c = make_ctx(devs[0], nullptr);
    if (!c) return 1;
    const int pr = write_preview(c);
    cvr_destroy(c);
    cvr_free_image(env_rgb);
    cvr_scene_destroy(scene);
    return pr;
  }
  if (filtered && !o.adaptive && o.iterations < 2) {
    fprintf(stderr, "[ConfigParser] Error: %s needs --iterations of at least 2 (a variance per pixel)\n",
            o.denoise ? "--denoise" : "--denoise-guided");
    return 2;
  }
  const bool tile_mode = ntiles > 1;
  if (n_dev > 1 && !tile_mode && (W % 8 || H % 8)) {
    printf("[Devices] one tile of %ux%u: block shards need sides that are multiples of 8; rendering on device %d\n", W,
           H, devs[0]);
    n_dev = 1;
  }
  if (n_dev > 1 && !tile_mode && o.rng_binding == "thread") {
    // the thread-bound RNG has no 8x8-block work order (cvr_render_share_to_host refuses it)
    printf("[Devices] --rng-binding thread renders paths in launch order, not in 8x8 blocks: no block shards; "
           "rendering on device %d\n", devs[0]);
    n_dev = 1;
  }
  if (n_dev > 1) {
    printf("[Devices] %zu contexts on devices", n_dev);
    for (int dv : devs) printf(" %d", dv);
    printf(": %s\n", tile_mode ? "tile k -> context k mod N" : "8x8-block shards of the image");
  }
  float* himg = nullptr;  // the shared pinned host image (multi-device)
  if (n_dev > 1 && cvr_host_alloc((size_t)W * H * 4 * sizeof(float), reinterpret_cast<void**>(&himg)) != CVR_OK) {
    fprintf(stderr, "Error: %s\n", cvr_last_error(nullptr));
    return 1;
  }
  cvr_render_desc d = {{W, H}, {o.tiles[0], o.tiles[1]}, o.iterations};
  for (unsigned t = 0; t < o.trials; ++t) {
    printf("---------------------------------------------------------------trial : %u \n", t);
    std::vector<cvr_ctx*> ctxs;
    for (size_t k = 0; k < n_dev; ++k) {
      cvr_ctx* share = nullptr;  // the first context on this device holds its medium
      for (size_t j = 0; j < k; ++j)
        if (devs[j] == devs[k]) {
          share = ctxs[j];
          break;
        }
      cvr_ctx* c = make_ctx(devs[k], share);
      if (!c) return 1;
      if (n_dev > 1 && !tile_mode && (r = cvr_set_block_shard(c, (uint32_t)k, (uint32_t)n_dev)) != CVR_OK) {
        fprintf(stderr, "Error: %s\n", cvr_last_error(c));
        return 1;
      }
      ctxs.push_back(c);
    }
    // (the first trial's render context: its build counted the kept voxels, no build of its own)
    if (t == 0 && o.field_stats && have_clip && print_kept(ctxs[0])) return 1;
    if (t == 0 && o.field_stats && have_labels && print_labels(ctxs[0])) return 1;
    cvr_stats st{};
    const auto t0 = std::chrono::steady_clock::now();
    cvr_adaptive_result ares{};
    std::vector<uint32_t> block_samples;
    std::vector<float> denoised;
    if (filtered) {
      // the session step by step, filtered (cvr_denoise / cvr_denoise_guided) before it ends.  Without --noise-target a
      // session that never stops a block: every block takes every sample, the plain render's
      // paths.  It takes two samples in its first pass and one in each later pass, so that no
      // launch adds more than two values into a pixel on top of nothing, or one on top of a sum:
      // the float atomics' arrival order then cannot change a bit (fp32 addition commutes, it
      // does not associate), and the sums, the image and the filtered image are the same bits in
      // every run.  One launch of all samples is faster and differs from run to run by an ulp in
      // a few pixels (profiles/denoise/README.md).
      cvr_ctx* c = ctxs[0];
      const cvr_adaptive_desc ad = o.adaptive ? cvr_adaptive_desc{o.min_iterations, o.iterations, o.pass_iterations,
                                                                  o.noise_target, 0.01f}
                                              : cvr_adaptive_desc{2u, o.iterations, 1u, -1.0f, 0.01f};
      const cvr_denoise_desc dd = {o.denoise_passes, o.denoise_sigma, 0.01f, 0u};
      block_samples.assign((size_t)(W / 8) * (H / 8), 0u);
      denoised.assign((size_t)W * H * 4, 0.0f);
      r = cvr_set_resolution(c, W, H);
      if (!r) r = cvr_set_offset(c, 0, 0);
      if (!r) r = cvr_adaptive_begin(c, &ad);
      while (!r && !ares.done) {
        cvr_stats ps{};
        if ((r = cvr_adaptive_pass(c, &ares)) || (r = cvr_get_stats(c, &ps))) break;
        st.paths += ps.paths;
        st.segments += ps.segments;
        st.steps += ps.steps;
        st.density += ps.density;
        st.albedo += ps.albedo;
        st.escaped += ps.escaped;
        st.truncated += ps.truncated;
        st.fetches += ps.fetches;
        st.kernel_ms += ps.kernel_ms;
      }
      if (!r) r = cvr_adaptive_image(c, image.data(), image.size());
      if (!r) r = cvr_adaptive_maps(c, nullptr, block_samples.data());
      if (!r && o.denoise) r = cvr_denoise(c, &dd, 0, denoised.data(), denoised.size());
      if (!r && o.denoise_guided) {
        const cvr_denoise_guided_desc gd = {dd, o.guide_sigma[0], o.guide_sigma[1], o.guide_sigma[2], 0u};
        const cvr_features_desc fd = {o.feature_step, 1.0f / 256.0f, 4096u, 0u};
        r = cvr_denoise_guided(c, &gd, &fd, 0, denoised.data(), denoised.size());
      }
      if (!r) r = cvr_adaptive_end(c);
      if (r != CVR_OK) {
        fprintf(stderr, "Error: %s\n", cvr_last_error(c));
        return 1;
      }
    } else if (o.adaptive) {
      // cvr_render_adaptive's steps, with the samples map read before the session ends
      cvr_ctx* c = ctxs[0];
      const cvr_adaptive_desc ad = {o.min_iterations, o.iterations, o.pass_iterations, o.noise_target, 0.01f};
      block_samples.assign((size_t)(W / 8) * (H / 8), 0u);
      r = cvr_set_resolution(c, W, H);
      if (!r) r = cvr_set_offset(c, 0, 0);
      if (!r) r = cvr_render_adaptive(c, &ad, image.data(), image.size(), &ares, &st);
      if (!r) r = cvr_adaptive_maps(c, nullptr, block_samples.data());
      if (r != CVR_OK) {
        fprintf(stderr, "Error: %s\n", cvr_last_error(c));
        return 1;
      }
    } else if (n_dev == 1) {
      r = cvr_render_image(ctxs[0], &d, nullptr, image.data(), &st);
      if (r != CVR_OK) {
        fprintf(stderr, "Error: %s\n", cvr_last_error(ctxs[0]));
        return 1;
      }
    } else {
      std::fill(himg, himg + (size_t)W * H * 4, 0.0f);  // pixels no tile covers stay 0 (Q1)
      std::vector<cvr_stats> sts(n_dev);
      std::vector<int> rcs(n_dev, CVR_OK);
      std::vector<std::string> errs(n_dev);
      std::vector<std::thread> th;
      for (size_t k = 0; k < n_dev; ++k)
        th.emplace_back([&, k] {
          rcs[k] = cvr_render_share_to_host(ctxs[k], &d, tile_mode ? (uint32_t)k : 0u, tile_mode ? (uint32_t)n_dev : 1u,
                                            himg, (size_t)W * H * 4, &sts[k]);
          if (rcs[k] != CVR_OK) errs[k] = cvr_last_error(ctxs[k]);
        });
      for (auto& x : th) x.join();
      for (size_t k = 0; k < n_dev; ++k) {
        if (rcs[k] != CVR_OK) {
          fprintf(stderr, "Error (context %zu, device %d): %s\n", k, devs[k], errs[k].c_str());
          return 1;
        }
        // every counter summed, as cvr_render_tiles sums its tiles'
        st.paths += sts[k].paths;
        st.segments += sts[k].segments;
        st.steps += sts[k].steps;
        st.density += sts[k].density;
        st.albedo += sts[k].albedo;
        st.escaped += sts[k].escaped;
        st.truncated += sts[k].truncated;
        st.fetches += sts[k].fetches;
        st.words += sts[k].words;
        st.iterations += sts[k].iterations;
        st.track_ms += sts[k].track_ms;
        st.events_ms += sts[k].events_ms;
        st.kernel_ms = std::max(st.kernel_ms, sts[k].kernel_ms);
      }
    }
    const auto t1 = std::chrono::steady_clock::now();
    if (n_dev > 1) std::copy(himg, himg + (size_t)W * H * 4, image.begin());
    const double sec = std::chrono::duration<double>(t1 - t0).count();
    printf("rendering time      : %.2f sec \n", sec);
    printf("total traced rays %llu (woodcock steps %llu)\n", (unsigned long long)st.segments,
           (unsigned long long)st.steps);
    if (o.adaptive) {
      const unsigned long long uniform = (unsigned long long)W * H * o.iterations;
      printf("adaptive render     : %u passes, %llu paths traced (%.1f%% of the uniform render's %llu), "
             "max block error %.6g, mean %.6g\n",
             ares.passes, (unsigned long long)ares.paths, 100.0 * (double)ares.paths / (double)uniform, uniform,
             ares.max_error, ares.mean_error);
      // the samples map, one grey value per pixel of its block, normalised by the maximum
      uint32_t smax = 1;
      for (uint32_t v : block_samples) smax = std::max(smax, v);
      std::vector<float> smap((size_t)W * H * 4, 1.0f);
      for (unsigned y = 0; y < H; ++y)
        for (unsigned x = 0; x < W; ++x) {
          const float v = (float)block_samples[(size_t)(y / 8) * (W / 8) + x / 8] / (float)smax;
          for (int ch = 0; ch < 3; ++ch) smap[((size_t)y * W + x) * 4 + ch] = v;
        }
      if (cvr_write_hdr((o.output + "_samples.hdr").c_str(), smap.data(), W, H) != CVR_OK) {
        fprintf(stderr, "Error: could not write %s_samples.hdr\n", o.output.c_str());
        return 1;
      }
    }
    std::vector<float> feat, feat_depth;
    if (o.features) {  // the guide buffers of the same view: one more pass over the medium, no samples
      const cvr_features_desc fd = {o.feature_step, 1.0f / 256.0f, 4096u, 0u};
      feat.assign((size_t)W * H * 4, 0.0f);
      feat_depth.assign((size_t)W * H, 0.0f);
      r = cvr_set_resolution(ctxs[0], W, H);
      if (!r) r = cvr_set_offset(ctxs[0], 0, 0);
      if (!r) r = cvr_features(ctxs[0], &fd, feat.data(), feat_depth.data(), feat.size());
      if (r != CVR_OK) {
        fprintf(stderr, "Error: %s\n", cvr_last_error(ctxs[0]));
        return 1;
      }
    }
    if (preview && t == 0 && write_preview(ctxs[0])) return 1;
    struct cvr_medium_info mi;
    if (cvr_medium_info(ctxs[0], &mi) == CVR_OK)
      printf("medium on device    : %s, %llu bytes (density %llu, cells %llu, albedo %llu, bounds %llu)\n",
             mi.format == CVR_FORMAT_F16 ? "half" : "float", (unsigned long long)mi.total_bytes,
             (unsigned long long)mi.density_bytes, (unsigned long long)mi.cells_bytes,
             (unsigned long long)mi.albedo_bytes, (unsigned long long)mi.bounds_bytes);
    if (t > 0) {
      times.push_back(sec);
      mean += sec;
    }
    for (size_t k = n_dev; k-- > 0;) cvr_destroy(ctxs[k]);  // sharers before the medium's owner
    cvr_write_hdr((o.output + ".hdr").c_str(), image.data(), W, H);
    if (o.pfm && write_pfm(o.output + ".pfm", image.data(), W, H)) {
      fprintf(stderr, "Error: could not write %s.pfm\n", o.output.c_str());
      return 1;
    }
    if (o.features) {
      // albedo as it is; opacity and depth as grey images (the scalar in all three channels)
      std::vector<float> plane((size_t)W * H * 4, 1.0f);
      const char* names[3] = {"_albedo", "_alpha", "_depth"};
      for (int k = 0; k < 3; ++k) {
        for (size_t i = 0; i < (size_t)W * H; ++i)
          for (int ch = 0; ch < 3; ++ch)
            plane[4 * i + ch] = k == 0 ? feat[4 * i + ch] : k == 1 ? feat[4 * i + 3] : feat_depth[i];
        if (cvr_write_hdr((o.output + names[k] + ".hdr").c_str(), plane.data(), W, H) != CVR_OK ||
            (o.pfm && write_pfm(o.output + names[k] + ".pfm", plane.data(), W, H))) {
          fprintf(stderr, "Error: could not write %s%s.hdr%s\n", o.output.c_str(), names[k], o.pfm ? " / .pfm" : "");
          return 1;
        }
      }
    }
    if (filtered && (cvr_write_hdr((o.output + "_denoised.hdr").c_str(), denoised.data(), W, H) != CVR_OK ||
                      (o.pfm && write_pfm(o.output + "_denoised.pfm", denoised.data(), W, H)))) {
      fprintf(stderr, "Error: could not write %s_denoised.hdr%s\n", o.output.c_str(), o.pfm ? " / .pfm" : "");
      return 1;
    }
  }
  if (himg) cvr_host_free(himg);
  cvr_free_image(env_rgb);
  if (o.trials > 1) {
    mean /= (double)times.size();
    double var = 0;
    for (double x : times) var += (x - mean) * (x - mean);
    var /= (double)times.size();
    printf("execution mean time of %.2f sec on %zu iterations and std %.5f \n", mean, times.size(), std::sqrt(var));
    printf("paths per sec %lf \n", (double)W * H * o.iterations / mean);
  }
  cvr_scene_destroy(scene);
  return 0;
}
