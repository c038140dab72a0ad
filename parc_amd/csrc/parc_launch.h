// The launch-status check of every launcher: return the HIP error of the launch(es) just issued from the enclosing entry point.
// And the grid of a grid-stride kernel: ceil(n / 256) workgroups of 256 threads, `cap` at the most.  Host only.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

static inline unsigned parc_capped_blocks(size_t n, size_t cap) {
    const size_t blocks = (n + 255) / 256;
    return (unsigned)(blocks > cap ? cap : blocks);
}

#define PARC_CHECK_LAUNCH()                         \
    do {                                            \
        hipError_t _e = hipGetLastError();          \
        if (_e != hipSuccess) return (int)_e;       \
    } while (0)
