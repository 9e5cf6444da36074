// ivf_error.h -- the error channel of the inverted-file sources (ivf_ann.hip, ivfpq_ann.hip through ivf_core.h; opq_ann.hip,
// refine_ann.hip): the message of the last failure on this thread, fail(), ITRY for a HIP call and ABI_CATCH for the end
// of a C entry point.  Everything is file-local: each source that includes this has its own g_err, which its own
// *_last_error() returns.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ivf_ann.h"
#include "abi_guard.h"
#define ABI_CATCH catch (...) { return abi_guard::caught(fail, IVF_ENOMEM, IVF_EINTERNAL); }

namespace {

thread_local std::string g_err;
int fail(int code, const std::string &m) {
  g_err = m;
  return code;
}
#define ITRY(expr)                                                                                \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess) return fail(IVF_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

}  // namespace
