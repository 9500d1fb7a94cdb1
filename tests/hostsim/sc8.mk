# The CPU build of the device control code (Makefile, hostsim.cpp) once more, with room for 8 entries of each map in the staging arrays of k_sc_rows
# (armada_amd/csrc/kernels_shapes_compact.h): small shape tables sit on both sides of the capacity (tests/test_z_shapes_compact.py).  A makefile of its own, with the
# flags of the Makefile beside it:   make -f sc8.mk
CXX ?= g++
CSRC := ../../armada_amd/csrc
DEPS := hostsim.cpp fast_serial.h fast_serial_engine.h $(wildcard $(CSRC)/*.h) $(wildcard $(CSRC)/*.inc) ../../include/armada_sched.h
FLAGS := -I. -O1 -g -std=c++17 -fPIC -ffp-contract=off -fno-strict-aliasing -Wall -Wno-unused-function -shared -pthread
libhostsim_sc8.so: $(DEPS)
	$(CXX) $(FLAGS) -DSC_LDS_CAP=8 -o $@ hostsim.cpp
