// Stand-in for <optixu/optixu_math_namespace.h>: see ref_shim_core.h (test infrastructure, no reference text).
#include "../ref_shim_core.h"
