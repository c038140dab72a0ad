// Heightfield cell lookup on a parc_terrain_t, for the device (the heightmap gathers and the tracker step through parc_hf_lookup.h, the
// generator call through parc_mdm_gen_core.h) and for the host builds of the shared cores.  No HIP in it.
#pragma once
#include <math.h>

#include "../../include/parc_hip.h"

#if defined(__HIPCC__)
#define PARC_HF_FN __device__ __forceinline__
#else
#define PARC_HF_FN static inline
#endif

// util/terrain_util.py:107-126: torch.round (half to even) then clamp to the grid
PARC_HF_FN float hf_lookup(const parc_terrain_t &t, float px, float py) {
    float fi = rintf((px - t.min_x) / t.dx);
    float fj = rintf((py - t.min_y) / t.dy);
    fi = fminf(fmaxf(fi, 0.f), (float)(t.dim_x - 1));
    fj = fminf(fmaxf(fj, 0.f), (float)(t.dim_y - 1));
    return t.hf[(int)fi * t.dim_y + (int)fj];
}
