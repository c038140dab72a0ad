// Heightfield cell lookup (hf_lookup: parc_hf_cell.h, which the host builds read too) and the per-env affine maps of the heightmap
// gather, shared by the stand-alone gather (parc_hfgather.hip) and the tracker step's heightmap wave and height termination
// (parc_kin.hip).  Device only.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/parc_hip.h"
#include "parc_hf_cell.h"
#include "parc_math.h"

struct hf_env_prm {
    float ax, bx, cx, ay, by, cy, gz;
};

template <bool FROM_STATE>
PARC_DEV hf_env_prm hf_env_params(int e, const float *__restrict__ root, const float *__restrict__ aux, const parc_terrain_t &ter,
                                  float inv_dx, float inv_dy) {
    float gx, gy, gz, c, s;
    if (FROM_STATE) {
        // ig_parkour_env.py:640-641: global xyz = root pos + env offset; heading of R(q) e_x (torch_util.py:470-479)
        const float *rs = root + (size_t)e * 13;
        gx = rs[0] + aux[3 * e + 0];
        gy = rs[1] + aux[3 * e + 1];
        gz = rs[2] + aux[3 * e + 2];
        float qx = rs[3], qy = rs[4], qz = rs[5], qw = rs[6];
        float a = 1.0f - 2.0f * (qy * qy + qz * qz);
        float b = 2.0f * (qw * qz + qx * qy);
        float n2 = a * a + b * b;
        float inv = rsqrtf(n2);
        c = n2 > 0.f ? a * inv : 1.0f;   // atan2(0,0) = 0
        s = n2 > 0.f ? b * inv : 0.0f;
    } else {
        gx = root[3 * e + 0];
        gy = root[3 * e + 1];
        gz = root[3 * e + 2];
        sincosf(aux[e], &s, &c);
    }
    hf_env_prm p;
    p.ax = c * inv_dx;
    p.bx = -s * inv_dx;
    p.cx = (gx - ter.min_x) * inv_dx;
    p.ay = s * inv_dy;
    p.by = c * inv_dy;
    p.cy = (gy - ter.min_y) * inv_dy;
    p.gz = gz;
    return p;
}
