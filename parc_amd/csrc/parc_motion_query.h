// A clip's frame pair at a time and what is blended from it (MotionLib.calc_motion_frame), shared by the stand-alone query
// (parc_motion.hip) and the tracker step (parc_kin.hip).  Device only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/parc_hip.h"
#include "parc_math.h"

struct frame_query {
    const float *row0, *row1;
    float blend, loop_phase;
    int wrap, idx0, idx1;     // idx = absolute frame row
};

// anim/motion_lib.py:443-456,527-538 (+ :458-475 loop offset)
PARC_DEV frame_query make_query(const parc_motion_lib_t &ml, int64_t id, float time) {
    frame_query fq;
    float len = ml.length[id];
    fq.wrap = ml.loop_mode[id] == 1;
    float phase = time / len;
    fq.loop_phase = floorf(phase);
    if (fq.wrap) phase = phase - floorf(phase);
    phase = fminf(fmaxf(phase, 0.f), 1.f);
    int nf = ml.num_frames[id];
    float fp = phase * (float)(nf - 1);
    int i0 = (int)fp;
    int i1 = min(i0 + 1, nf - 1);
    fq.blend = fp - (float)i0;
    int st = ml.start_idx[id];
    fq.idx0 = st + i0;
    fq.idx1 = st + i1;
    fq.row0 = ml.frames + (size_t)fq.idx0 * ml.row_stride;
    fq.row1 = ml.frames + (size_t)fq.idx1 * ml.row_stride;
    return fq;
}

// lane b: slerped quaternion b of the frame pair (b = 0 root rotation, b >= 1 joint b-1)
PARC_DEV q4 query_quat(const frame_query &fq, int b) {
    float4 a = *reinterpret_cast<const float4 *>(fq.row0 + 4 * b);
    float4 c = *reinterpret_cast<const float4 *>(fq.row1 + 4 * b);
    return slerp(mk4(a.x, a.y, a.z, a.w), mk4(c.x, c.y, c.z, c.w), fq.blend);
}

PARC_DEV float lerp_ref(float a, float b, float t) { return (1.0f - t) * a + t * b; }

PARC_DEV v3 query_root_pos(const parc_motion_lib_t &ml, const frame_query &fq, int64_t id) {
    const float *p0 = fq.row0 + ml.off_pos, *p1 = fq.row1 + ml.off_pos;
    v3 p = mk3(lerp_ref(p0[0], p1[0], fq.blend), lerp_ref(p0[1], p1[1], fq.blend), lerp_ref(p0[2], p1[2], fq.blend));
    if (fq.wrap) {
        const float *d = ml.pos_delta + 3 * id;
        p = p + mk3(fq.loop_phase * d[0], fq.loop_phase * d[1], fq.loop_phase * d[2]);
    }
    return p;
}
