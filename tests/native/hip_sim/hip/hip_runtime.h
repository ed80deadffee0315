// TEST INFRASTRUCTURE: stands in for <hip/hip_runtime.h> when a kernel file of the product is compiled for the CPU
// (tests/native/blockfind_sim.cpp, with -I tests/native/hip_sim): the device language comes from tests/native/hip_cpu_shim.h.
#ifndef NXZ_HIP_SIM_RUNTIME_H
#define NXZ_HIP_SIM_RUNTIME_H
#include "../../hip_cpu_shim.h"
#endif
