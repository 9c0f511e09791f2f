# How every HIP library of the package is built for gfx950 (MI355X); hipcc cross-compiles without a GPU.  Included by the Makefile
# of a source directory, which sets LIB (the library, ../libmobgt_<name>.so), SRCS (its .hip files), DEPS (the headers every object
# depends on) and, if it needs any, EXTRA_CXXFLAGS.
# -amdgpu-mfma-vgpr-form: keep MFMA accumulators in VGPRs (gfx950 has a unified register file); without it
# the compiler parks C/D in AGPRs and pays a v_accvgpr_read/write per element around every softmax step.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
CXXFLAGS ?= -O3 -std=c++17 -fPIC -I../../include --offload-arch=$(ARCH) -Wall -Wno-unused-function -mllvm -amdgpu-mfma-vgpr-form=1 -fno-slp-vectorize $(EXTRA_CXXFLAGS)
OBJS := $(SRCS:.hip=.o)
.DEFAULT_GOAL := all

all: $(LIB)

%.o: %.hip $(DEPS) Makefile ../hip.mk
	$(HIPCC) $(CXXFLAGS) -c $< -o $@

$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS)

clean:
	rm -f $(OBJS) $(LIB)
