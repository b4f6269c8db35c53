# Builds the product library kopia_amd/libkcdc.so (gfx950 only) and the C
# oracle used by the tests (oracle/_build/liboracle.so).
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
HIPFLAGS ?= -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Wall -Wno-unused-function
CSRC := kopia_amd/csrc
OBJ := build/obj
SRCS := $(CSRC)/kcdc_kernels.hip $(CSRC)/kcdc_hash.hip $(CSRC)/kcdc_crypt.hip $(CSRC)/kcdc_compress.hip $(CSRC)/kcdc_decompress.hip $(CSRC)/kcdc_inflate.hip $(CSRC)/kcdc_zstd.hip $(CSRC)/kcdc_ecc.hip $(CSRC)/kcdc_pack.hip $(CSRC)/kcdc_dedup.hip $(CSRC)/kcdc_api.cpp $(CSRC)/kcdc_writer.cpp $(CSRC)/kcdc_tables.cpp $(CSRC)/kcdc_registry.cpp
OBJS := $(patsubst $(CSRC)/%,$(OBJ)/%.o,$(SRCS))
LIB := kopia_amd/libkcdc.so

all: $(LIB) oracle build/writer_bench build/s2_decode_host build/inflate_host build/zstd_decode_host build/pack_plan_host build/dedup_host

# every object depends on every header of the sources' directory: a header edit rebuilds
HDRS := $(wildcard $(CSRC)/*.h) include/kcdc.h

$(OBJ)/%.hip.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(OBJ)/%.cpp.o: $(CSRC)/%.cpp $(HDRS)
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

$(LIB): $(OBJS)
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -o $@ $(OBJS)

oracle:
	$(MAKE) -s -C oracle

asm: $(CSRC)/kcdc_kernels.hip $(HDRS)
	@mkdir -p build/asm
	$(HIPCC) $(HIPFLAGS) --cuda-device-only -S $< -o build/asm/kcdc_kernels.s -Rpass-analysis=kernel-resource-usage 2> build/asm/resource.txt

clean:
	rm -rf build $(LIB)
	$(MAKE) -s -C oracle clean

# Instrumented builds for tools/debug_pipe.py (queue invariants, KCDC_DEBUG_CHECKS) and
# tools/trace_pipe.py (per-wave s_memrealtime trace, KCDC_TRACE); not used by the product.
build/libkcdc_dbg.so build/libkcdc_trace.so: $(SRCS) $(HDRS)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) $(if $(findstring dbg,$@),-DKCDC_DEBUG_CHECKS=1,-DKCDC_TRACE=1) -shared -o $@ \
	  $(filter %.hip,$(SRCS)) -x hip $(filter %.cpp,$(SRCS))
instrumented: build/libkcdc_dbg.so build/libkcdc_trace.so
.PHONY: instrumented

# C ABI driver: concurrent writers through grouped vs private streaming handles
build/group_bench: tools/group_bench.cpp include/kcdc.h $(LIB)
	@mkdir -p build
	g++ -O2 -std=c++17 -pthread -Iinclude $< -Lkopia_amd -lkcdc -Wl,-rpath,'$$ORIGIN/../kopia_amd' -o $@

.PHONY: all oracle clean asm

# ---- experiment builds (A/B of compile-time tunables through tools/kbench.py; not the product)
# e.g. make variants VARIANTS="base: diag:-DKCDC_HELP_DIAG=1"  (name:flags, flags comma-separated;
# the batch kernels' tunables are constants now: a variant of one is a patched source tree built here)
VARIANTS ?=
variants:
	@mkdir -p build/variants
	@for v in $(VARIANTS); do \
	  n=$${v%%:*}; f=$$(echo $${v#*:} | tr ',' ' '); \
	  echo "variant $$n: $$f"; \
	  $(HIPCC) $(HIPFLAGS) $$f -shared -o build/variants/libkcdc_$$n.so $(filter %.hip,$(SRCS)) -x hip $(filter %.cpp,$(SRCS)) || exit 1; \
	done
.PHONY: variants

# C ABI driver: batching object writers (kcdc_bw_*), aggregate host-to-cuts rate
build/writer_bench: tools/writer_bench.cpp include/kcdc.h $(LIB)
	@mkdir -p build
	g++ -O2 -std=c++17 -pthread -Iinclude $< -Lkopia_amd -lkcdc -Wl,-rpath,'$$ORIGIN/../kopia_amd' -o $@

# The S2 decoder's validity header on the CPU under the host sanitizers (tests/test_s2_vectors.py
# runs every vector through it before the GPU sees one)
build/s2_decode_host: tools/s2_decode_host.cpp $(CSRC)/kcdc_s2_format.h $(CSRC)/kcdc_wave.h
	@mkdir -p build
	g++ -std=c++17 -g -O1 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -I$(CSRC) $< -o $@

# The inflate decoder's validity header on the CPU under the host sanitizers
# (tests/test_inflate_vectors.py runs every vector through it before the GPU sees one)
build/inflate_host: tools/inflate_host.cpp $(CSRC)/kcdc_inflate_format.h
	@mkdir -p build
	g++ -std=c++17 -g -O1 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -I$(CSRC) $< -o $@

# The zstd decoder's validity header on the CPU under the host sanitizers
# (tests/test_zstd_vectors.py runs every vector through it before the GPU sees one)
build/zstd_decode_host: tools/zstd_decode_host.cpp $(CSRC)/kcdc_zstd_format.h
	@mkdir -p build
	g++ -std=c++17 -g -O1 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -I$(CSRC) $< -o $@

# The pack plan's decisions (stored sizes, placement, bounds) on the CPU under the host sanitizers
# (tests/test_pack_model.py compares them with the literal loop of tests/pack_model.py)
build/pack_plan_host: tools/pack_plan_host.cpp $(CSRC)/kcdc_pack_format.h $(CSRC)/kcdc_internal.h
	@mkdir -p build
	g++ -std=c++17 -g -O1 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -I$(CSRC) $< -o $@

# The content-ID set's decisions (probe, outcome, commit, lookup, refusal) run sequentially on the CPU
# under the host sanitizers, every table of its exact size (tests/test_dedup_model.py compares them
# with the literal loop of tests/dedup_model.py)
build/dedup_host: tools/dedup_host.cpp $(CSRC)/kcdc_dedup_format.h $(CSRC)/kcdc_internal.h
	@mkdir -p build
	g++ -std=c++17 -g -O1 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -I$(CSRC) $< -o $@

# Microbenchmarks run by tools/gpu_session.sh (valu:, membench): standalone HIP programs
build/valu_rate: tools/valu_rate.hip
	@mkdir -p build
	$(HIPCC) -O3 -std=c++17 --offload-arch=$(ARCH) $< -o $@
build/membench: tools/membench.hip
	@mkdir -p build
	$(HIPCC) -O3 -std=c++17 --offload-arch=$(ARCH) $< -o $@
tools: build/valu_rate build/membench build/writer_bench
.PHONY: tools
