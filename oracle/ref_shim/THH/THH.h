// Stand-in for the long-removed THC umbrella header (hipify turns the reference's `#include <THC/THC.h>` into this
// path).  earth_mover_distance.cu uses two names from it, in its host wrappers only; both are mapped onto what the
// installed torch provides.  Our text - nothing of the reference or of the old THC is reproduced here.
#pragma once
#include <c10/hip/HIPException.h>
#include <c10/util/Exception.h>

#define CHECK_EQ(a, b) TORCH_CHECK((a) == (b), #a " != " #b)
#define THCudaCheck(expr) C10_HIP_CHECK(expr)
