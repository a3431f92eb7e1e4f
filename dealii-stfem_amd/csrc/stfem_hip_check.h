// How every unit of the library turns a failing HIP call or kernel launch into STFEM_ERR_HIP with its reason in the error
// record (stfem_error.h).  Included by the host-side units (stfem_internal.h) and by the kernel units (stfem_core.h).
#pragma once
#include "../../include/stfem.h"
#include "stfem_error.h"

#include <hip/hip_runtime_api.h>

// Returns STFEM_ERR_HIP from the calling function if a HIP runtime call fails, recording "<call>: <reason>".
#define STFEM_TRY(call)                                                                               \
  do {                                                                                                \
    hipError_t e_ = (call);                                                                           \
    if (e_ != hipSuccess) return stfem_set_error(STFEM_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
  } while (0)

// Around a sequence of kernel launches.  begin drops a stale sticky error of an unrelated earlier call; end reads the launch
// error (which resets it: read it once) and returns STFEM_OK, or STFEM_ERR_HIP with "<what>: <reason>" recorded.
static inline void stfem_launch_begin() { (void)hipGetLastError(); }
static inline int stfem_launch_end(const char *what)
{
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? STFEM_OK : stfem_set_error(STFEM_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}
