// device_buf.h -- Buf, the device buffer of the index sources (hnsw_ann.hip, dense_ann.hip, ann_by_id.hip and, through
// ivf_kernels.h, the inverted-file sources): an allocation that is kept while it is large enough.  `bytes` is the size of
// the allocation; after a successful reserve or grow_keep `p` is never null (a request for 0 bytes allocates 8), so a null
// pointer handed to a kernel as "absent" always comes from a flag of the index, never from a Buf.  A source includes this
// once; everything is file-local.
// Two look-alikes stay separate on purpose: sann_host::DevBuf (sann_host.h), whose `bytes` is the logical size, whose growth
// adds a quarter and whose alloc(0) leaves null, and the one-shot `put` buffer of rsx_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace {

struct Buf {
  void *p = nullptr;
  size_t bytes = 0;
  Buf() = default;
  Buf(const Buf &) = delete;
  Buf &operator=(const Buf &) = delete;
  ~Buf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  // room for n bytes; the contents are not kept when it grows
  hipError_t reserve(size_t n) {
    if (p && n <= bytes) return hipSuccess;
    release();
    hipError_t e = hipMalloc(&p, n ? n : 8);
    if (e == hipSuccess) bytes = n ? n : 8;
    return e;
  }
  // growth that keeps the first `keep` bytes (device to device); the old buffer goes only once the new one holds them
  hipError_t grow_keep(size_t keep, size_t want) {
    if (p && want <= bytes) return hipSuccess;
    void *np = nullptr;
    hipError_t e = hipMalloc(&np, want ? want : 8);
    if (e != hipSuccess) return e;
    if (keep && p) {
      e = hipMemcpy(np, p, keep, hipMemcpyDeviceToDevice);
      if (e != hipSuccess) {
        (void)hipFree(np);
        return e;
      }
    }
    if (p) (void)hipFree(p);
    p = np;
    bytes = want ? want : 8;
    return hipSuccess;
  }
  template <class T> T *as() const { return (T *)p; }
};

}  // namespace
