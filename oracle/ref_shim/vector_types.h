// Stand-in for <vector_types.h>: see ref_shim_core.h (test infrastructure, no reference text).
#include "ref_shim_core.h"
