// The launch-status check of every launcher: return the HIP error of the launch(es) just issued from the enclosing entry point.
// Host only.
#pragma once
#include <hip/hip_runtime.h>

#define PARC_CHECK_LAUNCH()                         \
    do {                                            \
        hipError_t _e = hipGetLastError();          \
        if (_e != hipSuccess) return (int)_e;       \
    } while (0)
