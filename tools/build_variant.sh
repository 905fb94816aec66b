#!/bin/bash
# tools/build_variant.sh NAME [-DFLAG ...] : an A/B build of the library as variants/lib_NAME.so (ABFT_HIP_LIB picks it up)
N=$1; shift
mkdir -p variants
# (trail_host.cpp: the protected trail's host functions, plain C++ as csrc/Makefile builds them; the variant's -D flags
# are the HIP sources')
cd abft_sparse_cg_amd/csrc && ${CXX:-g++} -O2 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unknown-pragmas \
  -c trail_host.cpp -o ../../variants/trail_host_$N.o && \
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -ffp-contract=off --offload-arch=gfx950 -Wall \
  -Wno-unused-function -shared "$@" -o ../../variants/lib_$N.so kernels.hip abft_hip.hip -Wl,../../variants/trail_host_$N.o
