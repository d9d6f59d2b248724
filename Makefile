# Build liborleans_route.so (HIP, gfx950) and the CPU oracle (test infrastructure).
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
HIPFLAGS = --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall -Wno-unused-function
CSRC = orleans_amd/csrc
# the device units (.hip), then the host units (.cpp); a new unit is one more name here
SRC = route_kernels.hip dir_mutate.hip cache_evict.hip cache_adaptive.hip dir_versions.hip admit.hip waitq.hip collect.hip \
      wire_codec.hip orl_api.cpp api_cache.cpp api_sw.cpp api_wire.cpp api_sched.cpp orl_node.cpp
OBJ = $(addprefix build/,$(addsuffix .o,$(basename $(SRC))))
LIB = orleans_amd/liborleans_route.so
# RCCL (the node exchange); inside a torch process the soname resolves to torch's loaded copy
LIBS = -L/opt/rocm/lib -Wl,-rpath,/opt/rocm/lib -lrccl

all: $(LIB) oracle

$(LIB): $(OBJ)
	$(HIPCC) --offload-arch=$(ARCH) -shared -o $@ $(OBJ) $(LIBS)

# headers: from the depfile the compiler writes beside each object
build/%.o: $(CSRC)/%.hip
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -MMD -MP -c -o $@ $<

build/%.o: $(CSRC)/%.cpp
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -MMD -MP -x hip -c -o $@ $<

-include $(OBJ:.o=.d)

oracle:
	$(MAKE) -C oracle

# A/B build of the kernels with extra defines, for the lab scripts only (LAB_LIB=lab/liborleans_route_<NAME>.so):
#   make lab NAME=fan512 DEFS=-DORL_FAN_LDS=512
lab: $(filter-out build/route_kernels.o,$(OBJ))
	@mkdir -p build lab
	$(HIPCC) $(HIPFLAGS) $(DEFS) -c -o build/route_kernels_$(NAME).o $(CSRC)/route_kernels.hip
	$(HIPCC) --offload-arch=$(ARCH) -shared -o lab/liborleans_route_$(NAME).so build/route_kernels_$(NAME).o \
		$(filter-out build/route_kernels.o,$(OBJ)) $(LIBS)

clean:
	rm -rf build $(LIB)
	$(MAKE) -C oracle clean

.PHONY: all oracle clean lab
