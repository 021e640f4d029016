# Build of the MI355X volumetric path tracer (gfx950 only).
#   make            -> cudavolumerenderer_amd/libcvr.so + cudavolumerenderer_amd/cvr (CLI)
#   make oracle     -> oracle/liboracle.so (test infrastructure)
# -ffp-contract=off: the kernels must perform exactly the IEEE operations of
# the source (see include/cvr_detmath.h); the correctly-rounded fp32 divide /
# sqrt flag is the hipcc default, spelled out because parity depends on it.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
PKG := cudavolumerenderer_amd
CSRC := $(PKG)/csrc
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off \
            -fhip-fp32-correctly-rounded-divide-sqrt -Iinclude -I$(CSRC) -Wall
OBJDIR ?= build/obj
SRCS_HIP := $(CSRC)/cvr_kernels.hip $(CSRC)/cvr_persistent.hip $(CSRC)/cvr_pool.hip $(CSRC)/cvr_wpool.hip $(CSRC)/cvr_wavefront.hip \
            $(CSRC)/cvr_denoise.hip $(CSRC)/cvr_medium_build.hip $(CSRC)/cvr_env.hip $(CSRC)/cvr_features.hip $(CSRC)/cvr_field.hip $(CSRC)/cvr_preview.hip $(CSRC)/cvr_shadow.hip $(CSRC)/cvr_project.hip
SRCS_CPP := $(CSRC)/cvr_api.cpp $(CSRC)/cvr_launch.cpp $(CSRC)/cvr_frame.cpp $(CSRC)/cvr_adaptive.cpp \
            $(CSRC)/cvr_denoise_api.cpp $(CSRC)/cvr_medium.cpp $(CSRC)/cvr_environment.cpp $(CSRC)/cvr_features_api.cpp $(CSRC)/cvr_preview_api.cpp $(CSRC)/cvr_shadow_api.cpp $(CSRC)/cvr_field_api.cpp $(CSRC)/cvr_project_api.cpp $(CSRC)/cvr_image_io.cpp $(CSRC)/cvr_scene.cpp $(CSRC)/cvr_vdb.cpp $(CSRC)/cvr_mhd.cpp $(CSRC)/cvr_xml.cpp
OBJS := $(patsubst $(CSRC)/%.hip,$(OBJDIR)/%.o,$(SRCS_HIP)) $(patsubst $(CSRC)/%.cpp,$(OBJDIR)/%.o,$(SRCS_CPP))
HDRS := include/cvr.h include/cvr_detmath.h $(wildcard $(CSRC)/*.h)
# Per-file flags, HIPFLAGS_<file name without .hip>; every rule that compiles a .hip file goes through
# hipflags, so the library, `variant`, `stamps`, `resource-usage` and `census-asm` agree.
# cvr_wpool.hip, SLP vectorisation off: at -O3 the SLP vectoriser pairs adjacent fp32 multiplies, adds
# and fmas of k_wpool into v_pk_{mul,add,fma}_f32.  A wave64 fp32 op already issues at the SIMD's whole
# fp32 rate, so a packed op does two ops' work in no less than two ops' time; what the packing adds is
# the moves that assemble register pairs, SALU and SGPR spill traffic (DESIGN.md §3.2, §8;
# profiles/round7/README.md).  Packed and plain ops are the same IEEE operations per component, so
# results do not change; tests/test_wpool_unpacked.py fails if the packing comes back.
HIPFLAGS_cvr_wpool := -fno-slp-vectorize
hipflags = $(HIPFLAGS) $(HIPFLAGS_$(basename $(notdir $(1)))) $(DEFS)

all: $(PKG)/libcvr.so $(PKG)/cvr build/launcher_order build/wpool_select build/wpool_select_env build/regen_plan oracle

$(OBJDIR)/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(call hipflags,$<) -c $< -o $@

$(OBJDIR)/%.o: $(CSRC)/%.cpp $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(call hipflags,$<) -x hip -c $< -o $@

$(PKG)/libcvr.so: $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS) -Wl,-soname,libcvr.so -lz

$(PKG)/cvr: $(CSRC)/cvr_main.cpp $(PKG)/libcvr.so include/cvr.h
	g++ -O2 -std=c++17 -Iinclude -o $@ $< -L$(PKG) -lcvr -Wl,-rpath,'$$ORIGIN'

# Host-only C++ test: libcvr driven through include/cvr_launcher.hpp in
# CudaVolPath's call order (tests/test_launcher_adapter.py).
build/launcher_order: tests/cpp/launcher_order.cpp include/cvr_launcher.hpp include/cvr.h $(PKG)/libcvr.so
	@mkdir -p build
	g++ -O2 -std=c++17 -Wall -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include -o $@ $< \
	    -L$(PKG) -lcvr -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,'$$ORIGIN/../$(PKG)' -Wl,-rpath,/opt/rocm/lib

# Host-only C++ test: the wave pool's instance selection over its whole request space
# (tests/test_wpool_select.py); no HIP.
build/wpool_select: tests/cpp/wpool_select.cpp $(CSRC)/cvr_wpool_select.h
	@mkdir -p build
	g++ -O2 -std=c++17 -Wall -Wextra -I$(CSRC) -o $@ $<
# The same over the environment half of the space (tests/test_wpool_select_env.py)
build/wpool_select_env: tests/cpp/wpool_select_env.cpp $(CSRC)/cvr_wpool_select.h
	@mkdir -p build
	g++ -O2 -std=c++17 -Wall -Wextra -I$(CSRC) -o $@ $<

# Host-only C++ test: the regeneration burst's bookkeeping against a unit-by-unit model
# (tests/test_regen_plan.py); no HIP.
build/regen_plan: tests/cpp/regen_plan.cpp $(CSRC)/cvr_regen_plan.h
	@mkdir -p build
	g++ -O2 -std=c++17 -Wall -Wextra -I$(CSRC) -o $@ $<
# The same program under AddressSanitizer and UBSan, run once (a CPU run)
regen-plan-asan: tests/cpp/regen_plan.cpp $(CSRC)/cvr_regen_plan.h
	@mkdir -p build/asan
	g++ -O1 -g -std=c++17 -Wall -Wextra -I$(CSRC) -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    -o build/asan/regen_plan $<
	build/asan/regen_plan
.PHONY: regen-plan-asan

oracle:
	$(MAKE) -C oracle

resource-usage:
	$(foreach f,$(SRCS_HIP),$(HIPCC) $(call hipflags,$(f)) -Rpass-analysis=kernel-resource-usage -c $(f) -o /dev/null &&) true

# Device assembly of the wave-pool kernels with line tables, the input of tools/isa_census.py
census-asm: build/census/cvr_wpool.s
build/census/cvr_wpool.s: $(CSRC)/cvr_wpool.hip $(HDRS)
	@mkdir -p build/census
	$(HIPCC) $(call hipflags,$<) -gline-tables-only --cuda-device-only -S $< -o $@

clean:
	rm -rf build $(PKG)/libcvr.so $(PKG)/cvr
	$(MAKE) -C oracle clean

.PHONY: all oracle clean resource-usage census-asm

# Diagnostic build with in-kernel phase stamps (never the shipped library).
stamps:
	$(MAKE) OBJDIR=build/stamps/obj DEFS=-DCVR_STAMPS=1 build/stamps/libcvr.so
.PHONY: stamps

# Experiment builds: make variant NAME=u2 DEFS="-DCVR_WPOOL_UNROLL=2" -> build/variants/u2/libcvr.so
# (objects through the rules above in a directory of the build's own, so per-file flags hold; always from scratch)
variant:
	rm -rf build/variants/$(NAME)/obj
	$(MAKE) OBJDIR=build/variants/$(NAME)/obj DEFS="$(DEFS)" build/variants/$(NAME)/libcvr.so
.PHONY: variant
build/%/libcvr.so: $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS) -lz
# The denoiser with global-memory taps in every pass (the A/B partner of the LDS-staged steps 1 and
# 2: profiles/denoise/README.md); only cvr_denoise.hip differs from the in-tree library
variant-dnplain: $(OBJS)
	@mkdir -p build/variants/dnplain
	$(HIPCC) $(HIPFLAGS) -DCVR_DENOISE_LDS=0 -c $(CSRC)/cvr_denoise.hip -o build/variants/dnplain/cvr_denoise.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o build/variants/dnplain/libcvr.so \
	    $(filter-out $(OBJDIR)/cvr_denoise.o,$(OBJS)) build/variants/dnplain/cvr_denoise.o -Wl,-soname,libcvr.so -lz
.PHONY: variant-dnplain
# Host statements under AddressSanitizer and UBSan: the host code alone of the listed sources is
# compiled with the sanitizers (-Xarch_host: the device code is not) and linked with the library's
# other objects and a check program with a main of its own.  A CPU run, no GPU.  The loop over a
# voxel's neighbours (cvr_gradient.h) is compiled into cvr_medium.cpp and cvr_field_api.cpp.
#   $(1): the stem of <stem>-host-asan and tests/cpp/<stem>_host_check.cpp, $(2): the sources' names
define host_asan
$(1)-host-asan: $$(OBJS)
	@mkdir -p build/asan
	$$(foreach f,$(2),$$(HIPCC) $$(call hipflags,$$(CSRC)/$$(f).cpp) -O1 -g -Xarch_host -fsanitize=address,undefined \
	    -Xarch_host -fno-sanitize-recover=undefined -x hip -c $$(CSRC)/$$(f).cpp -o build/asan/$$(f).o &&) true
	g++ -O1 -g -std=c++17 -Wall -Iinclude -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    -c tests/cpp/$(1)_host_check.cpp -o build/asan/$(1)_host_check.o
	$$(HIPCC) --offload-arch=$$(ARCH) -fsanitize=address,undefined -o build/asan/$(1)_host_check \
	    build/asan/$(1)_host_check.o $$(filter-out $$(patsubst %,$$(OBJDIR)/%.o,$(2)),$$(OBJS)) \
	    $$(patsubst %,build/asan/%.o,$(2)) -lz
	build/asan/$(1)_host_check
.PHONY: $(1)-host-asan
endef
# cvr_classify_gradient_host and the gradient descriptor's checks
$(eval $(call host_asan,gradient,cvr_medium))
# cvr_features_host and cvr_denoise_guided_host
$(eval $(call host_asan,features,cvr_features_api cvr_denoise_api))
# cvr_field_stats_host and cvr_field_histogram_host
$(eval $(call host_asan,field,cvr_field_api))
# cvr_clip_host and the clip descriptor's checks
$(eval $(call host_asan,clip,cvr_medium))
# cvr_classify_labels_host and the labelled descriptor's checks
$(eval $(call host_asan,labels,cvr_medium))
# cvr_preview_host and the preview descriptor's checks (the march's checks are cvr_features_api.cpp's)
$(eval $(call host_asan,preview,cvr_preview_api cvr_features_api))
# cvr_light_volume_host, cvr_preview_shadowed_host and their descriptors' checks (the march's and the shading's
# checks are cvr_features_api.cpp's and cvr_preview_api.cpp's)
$(eval $(call host_asan,shadow,cvr_shadow_api cvr_preview_api cvr_features_api))
# cvr_field_project_host and the projection descriptor's checks
$(eval $(call host_asan,project,cvr_project_api))
