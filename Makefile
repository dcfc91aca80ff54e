# Build of the product libraries and the test oracle.  `python -c "import __graft_entry__ as g; g.build()"` runs this.
HIPCC    ?= /opt/rocm/bin/hipcc
CC       ?= gcc
ROOT     := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
LIBDIR   ?= actinon_amd/lib
BUILD    ?= build
CFLAGS   := -O2 -fPIC -std=gnu11 -Wall -Wno-unused-function -ffp-contract=off -Iinclude
SHADE_WAVES ?= 4
WALK_WAVES  ?= 4
# k_walk: 4 waves per SIMD (128 VGPRs) since round 4.  Rounds 2 - 3 ran it at 2 (256 VGPRs): with every operand of every pair
# expanded four times in line the kernel was 1.4 MB of code and spilled ~800 registers at 128.  With the operand loops of
# pair_hit, the roughness perturbation as a real call and one copy of the root traversal it is 140 KB, spills ~160 at 128, and
# the two extra waves per SIMD hide more latency than the spills add: 1080p 57.6 -> 53.0 ms, diamond -11 % (profiles/r04/)
TRACE_WAVES ?= 4
EXTRA_DEFS ?=
OPT ?= -O3
HIPFLAGS := $(EXTRA_DEFS) -DACN_SHADE_WAVES=$(SHADE_WAVES) -DACN_WALK_WAVES=$(WALK_WAVES) -DACN_TRACE_WAVES=$(TRACE_WAVES) $(OPT) -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -Iinclude -Iactinon_amd/csrc -std=c++17 -Wall -Wno-unused-function -Wno-unused-value -Wno-unused-result

all: hip host oracle cli

hip: $(LIBDIR)/libactinon_hip.so
host: $(LIBDIR)/libactinon_host.so
oracle: oracle/libacn_oracle.so oracle/libacn_oracle_libm.so
cli: actinon_amd/bin/actinon_hip

# one object per kernel family: `make -j` compiles them side by side (acn_launch.h)
HIP_UNITS := actinon_hip acn_calls k_query k_stage k_rays k_surface k_denoise k_denoise_layers k_fill k_lens k_lens_surface k_lens_layers k_lens_layers_merge k_reproject k_shadow k_select k_frame k_shade_64 k_shade_16 k_shade_4 k_shade_1 k_walk_lds k_walk_glb k_walk_count k_walk_count_prune k_hard_shadow k_hard_path
HIP_OBJS  := $(addprefix $(BUILD)/,$(addsuffix .o,$(HIP_UNITS)))
# the two production units of k_walk are scheduled for instruction-level parallelism: __launch_bounds__ fixes their occupancy
# (2 waves per SIMD), which is what the default strategy schedules for (hanging_lamp 600x800 -3 %, everything else equal:
# profiles/r03/ab_walk_max_ilp_scheduling.txt; same bits: scheduling does not reassociate)
WALK_SCHED ?= -mllvm -amdgpu-sched-strategy=max-ilp
$(BUILD)/k_walk_lds.o $(BUILD)/k_walk_glb.o: HIPFLAGS += $(WALK_SCHED)
# (dependencies on headers: as the compiler sees them, $(BUILD)/*.d)
$(BUILD)/%.o: actinon_amd/csrc/%.hip
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -MMD -MP -c -o $@ $<
# the scene tables of the upload: host-only C++, no HIP (tests/test_tables_cpu.py compiles the same unit on its own)
$(BUILD)/acn_tables.o: actinon_amd/csrc/acn_tables.cpp
	@mkdir -p $(BUILD)
	$(CXX) -O2 -fPIC -std=c++17 -Wall -ffp-contract=off -fno-fast-math -Iinclude -Iactinon_amd/csrc -MMD -MP -c -o $@ $<
-include $(HIP_OBJS:.o=.d) $(BUILD)/acn_tables.d
$(LIBDIR)/libactinon_hip.so: $(HIP_OBJS) $(BUILD)/acn_tables.o
	@mkdir -p $(LIBDIR)
	$(HIPCC) --offload-arch=gfx950 -shared -fPIC -o $@ $(HIP_OBJS) $(BUILD)/acn_tables.o

$(LIBDIR)/libactinon_host.so: actinon_amd/host/acn_scene.c actinon_amd/host/acn_driver.c actinon_amd/host/acn_scenes.c actinon_amd/host/acn_interp.c include/acn_scene.h include/acn_interp.h include/actinon_hip.h $(LIBDIR)/libactinon_hip.so
	$(CC) $(CFLAGS) -shared -o $@ actinon_amd/host/acn_scene.c actinon_amd/host/acn_driver.c actinon_amd/host/acn_scenes.c actinon_amd/host/acn_interp.c -L$(LIBDIR) -lactinon_hip -lm -Wl,-rpath,'$$ORIGIN'

actinon_amd/bin/actinon_hip: tools/actinon_hip.c include/acn_interp.h $(LIBDIR)/libactinon_host.so
	@mkdir -p actinon_amd/bin
	$(CC) $(CFLAGS) -o $@ tools/actinon_hip.c -L$(LIBDIR) -lactinon_host -lactinon_hip -lm -Wl,-rpath,'$$ORIGIN/../lib'

# the two prebuilt oracles travel to the GPU box: a portable ISA level (AVX2 + FMA), not the build container's -march=native
# (bench.py compiles a third build on the box itself with the reference's flags for the CPU baseline)
ORACLE_MARCH ?= x86-64-v3
oracle/libacn_oracle.so: oracle/acn_oracle.c oracle/acn_oracle.h actinon_amd/csrc/acn_detmath.h actinon_amd/csrc/acn_costs.h include/actinon_hip.h
	$(CC) $(CFLAGS) -march=$(ORACLE_MARCH) -Ioracle -shared -o $@ oracle/acn_oracle.c -lm -lpthread

oracle/libacn_oracle_libm.so: oracle/acn_oracle.c oracle/acn_oracle.h actinon_amd/csrc/acn_costs.h include/actinon_hip.h
	$(CC) $(CFLAGS) -march=$(ORACLE_MARCH) -DACN_ORACLE_LIBM -Ioracle -shared -o $@ oracle/acn_oracle.c -lm -lpthread

# Device code identity: per unit the SHA-256 of .text, of .rodata (- if none) and of the notes of its gfx950 code
# object, from the objects as they are (- - -: a unit without device code); equal lines before and after a change: the kernels are the same
LLVM_BIN ?= $(dir $(HIPCC))../lib/llvm/bin
digests:
	@t=$$(mktemp -d) && for u in $(HIP_UNITS); do \
	    if ! $(LLVM_BIN)/llvm-objcopy --dump-section .hip_fatbin=$$t/fb $(BUILD)/$$u.o $$t/o 2>/dev/null; then echo $$u - - -; continue; fi; \
	    $(LLVM_BIN)/clang-offload-bundler --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=$$t/fb --output=$$t/elf || exit 1; \
	    for s in text rodata; do $(LLVM_BIN)/llvm-objcopy -O binary --only-section=.$$s $$t/elf $$t/$$s || exit 1; done; \
	    $(LLVM_BIN)/llvm-readelf --notes $$t/elf > $$t/notes || exit 1; \
	    echo $$u $$(sha256sum < $$t/text | cut -c1-64) $$(if [ -s $$t/rodata ]; then sha256sum < $$t/rodata | cut -c1-64; else echo -; fi) $$(sha256sum < $$t/notes | cut -c1-64); \
	done; rm -rf $$t

clean:
	rm -rf build; rm -f $(LIBDIR)/*.so oracle/*.so actinon_amd/bin/actinon_hip

.PHONY: all hip host oracle cli clean digests
