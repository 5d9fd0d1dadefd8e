// The status of the launches a host driver has just made, as the C ABI reports it.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "plan.h"

namespace nqa {

inline int launch_status(const char* name) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error(std::string(name) + ": " + hipGetErrorString(e));
    return NQA_ERR_LAUNCH;
  }
  return NQA_OK;
}

}  // namespace nqa
