// rmpc_err.hpp -- the error channel of the library: the message rmpc_last_error() returns and the two ways the host
// code sets it.  Every translation unit shares it: rmpc_host.hpp includes it, rmpc_world.hip includes it directly.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

inline thread_local std::string g_err;   // (one object for all translation units of the library)
inline int fail(const std::string &m) {
  g_err = m;
  return -1;
}
#define HIPCHK(x)                                                                         \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess)                                                                 \
      return fail(std::string(#x) + ": " + hipGetErrorString(e_));                        \
  } while (0)
