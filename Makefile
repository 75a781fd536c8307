# Builds the gfx950 engine (C ABI) and the oracle's optional native bits.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
SRC := $(wildcard pycsou_amd/csrc/*.hip)
HDR := $(wildcard pycsou_amd/csrc/*.hpp) include/pycsou_hip.h
LIB := pycsou_amd/lib/libpycsou_hip.so
OBJ := $(patsubst pycsou_amd/csrc/%.hip,build/%.o,$(SRC))
FLAGS := --offload-arch=$(ARCH) -O3 -fno-slp-vectorize -fPIC -std=c++17 -Wall -Wno-unused-function -Iinclude
# mcmc.hip: running sums and P2 markers must round as NumPy does (no a*b+c -> fma)
FLAGS_mcmc := -ffp-contract=off
# cg.hip: the CG recurrences round as SciPy's do (p *= beta; p += r is two roundings)
FLAGS_cg := -ffp-contract=off

all: $(LIB)

build/%.o: pycsou_amd/csrc/%.hip $(HDR)
	@mkdir -p build
	$(HIPCC) $(FLAGS) $(FLAGS_$*) -c $< -o $@

$(LIB): $(OBJ)
	@mkdir -p pycsou_amd/lib
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJ) -L/opt/rocm/lib -lrocfft -Wl,-rpath,/opt/rocm/lib

clean:
	rm -rf build $(LIB)

.PHONY: all clean
