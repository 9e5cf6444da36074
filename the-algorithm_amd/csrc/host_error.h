// host_error.h -- the error channel of an index source (hnsw_ann.hip, dense_ann.hip, ann_by_id.hip and, through ivf_error.h,
// the inverted-file sources): the message of the last failure on this thread, fail(), and HIP_TRY_AS(code, expr) for a HIP
// call that returns the module's device code with the failed expression as the message.  Each source names its module once:
//   #define HTRY(e) HIP_TRY_AS(HNSW_EDEVICE, e)
//   #define ABI_CATCH catch (...) { return abi_guard::caught(fail, HNSW_ENOMEM, HNSW_EINTERNAL); }
// Everything is file-local: each source that includes this has its own g_err, which its own *_last_error() returns.  The
// SANN sources (sann_host::fail, shared across their translation units by design) and rsx_kernels.hip keep their own.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "abi_guard.h"

namespace {

thread_local std::string g_err;
int fail(int code, const std::string &m) {
  g_err = m;
  return code;
}
#define HIP_TRY_AS(code, expr)                                                                \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) return fail(code, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

}  // namespace
