// Stand-in for <cuda/helpers.h>: see ref_shim_core.h (test infrastructure, no reference text).
#include "../ref_shim_core.h"
