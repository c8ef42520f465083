# TEST INFRASTRUCTURE: tests/asan_small_launches.cpp as a stand-alone AddressSanitizer program -- the product's .hip sources,
# unchanged, against the fiber emulator in this directory, linked into one executable with its own main.  Nothing is preloaded.
# The objects are those of asan_compact.mk and asan_hist16.mk (same sources, same flags, same directory): whichever runs first
# builds them.
#     make -C tests/emu -f asan_small.mk [ASAN_CXX=g++]
ASAN_CXX ?= clang++
CSRC      = ../../suffix_amd/csrc
DIR       = asan/cp
PARTS     = radix sa tile tiny lcp tree query microbench api
OBJS      = $(addprefix $(DIR)/sfx_,$(addsuffix .o,$(PARTS))) $(DIR)/emu_runtime.o
HDRS      = $(wildcard $(CSRC)/*.hpp) $(wildcard $(CSRC)/*.hip) ../../include/suffix_hip.h hip/hip_runtime.h
FLAGS     = -O1 -g -std=c++17 -I. -DSFX_DEV_HOOKS -fsanitize=address -fno-omit-frame-pointer -Wno-unknown-pragmas

all: $(DIR)/asan_small_launches
$(DIR)/sfx_%.o: $(CSRC)/sfx_%.hip $(HDRS)
	@mkdir -p $(DIR)
	$(ASAN_CXX) $(FLAGS) -x c++ -c $< -o $@
$(DIR)/emu_runtime.o: emu_runtime.cpp hip/hip_runtime.h
	@mkdir -p $(DIR)
	$(ASAN_CXX) $(FLAGS) -c $< -o $@
$(DIR)/asan_small_launches: ../asan_small_launches.cpp $(OBJS)
	$(ASAN_CXX) $(FLAGS) -I../../include ../asan_small_launches.cpp $(OBJS) -o $@ -lpthread
clean:
	rm -f $(DIR)/asan_small_launches
