// ivf_error.h -- the error channel (host_error.h) as the inverted-file sources name it (ivf_ann.hip, ivfpq_ann.hip,
// grouped_ann.hip through ivf_core.h; opq_ann.hip, refine_ann.hip): ITRY for a HIP call and ABI_CATCH for the end of a C
// entry point, both with the IVF_* status codes.
#pragma once
#include "../../include/ivf_ann.h"
#include "host_error.h"
#define ITRY(expr) HIP_TRY_AS(IVF_EDEVICE, expr)
#define ABI_CATCH catch (...) { return abi_guard::caught(fail, IVF_ENOMEM, IVF_EINTERNAL); }
