// The per-sample device functions of the AMP observation side - whole, and in the parts a kernel may spread over lanes -
// shared by amp_obs.hip (whole batches), amp_reset.hip (the reset rows of an environment) and amp_demo.hip (the demo fetch): the motion-clip sampler (utils/motion_lib.py:122-172,263-272,296-325;
// utils/torch_utils.py:7-28,94-118) and one frame of the discriminator observation (env/tasks/humanoid_amp.py:280-316,
// env/tasks/humanoid.py:523-552).  All three compile with -ffp-contract=off: every expression rounds operation by operation.
#pragma once
#include "common.h"
#include "quat.h"

namespace {

constexpr int kMaxJoints = 32;

// the concatenated clip tensors of a motion library and the character's joint / key-body tables
struct MotionClips {
    const float *gts, *grs, *lrs, *grvs, *gravs, *dvs;       // [frames, B, 3] [frames, B, 4] x2 [frames, 3] x2 [frames, D]
    const float *lengths, *dt;                               // per motion
    const int32_t *num_frames, *length_starts;
    int B, D, J, K;
    int dof_off[kMaxJoints + 1], dof_body[kMaxJoints], key_body[kMaxJoints];
};

__device__ __forceinline__ Q4 slerp(const Q4& a, Q4 b, float t) {
    float c = a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
    if (c < 0.f) b = Q4{-b.x, -b.y, -b.z, -b.w};
    c = fabsf(c);
    if (c >= 1.f) return a;
    const float ht = acosf(c), s = sqrtf(1.f - c * c);
    if (fabsf(s) < 0.001f) return Q4{0.5f * a.x + 0.5f * b.x, 0.5f * a.y + 0.5f * b.y, 0.5f * a.z + 0.5f * b.z, 0.5f * a.w + 0.5f * b.w};
    const float ra = sinf((1.f - t) * ht) / s, rb = sinf(t * ht) / s;
    return Q4{ra * a.x + rb * b.x, ra * a.y + rb * b.y, ra * a.z + rb * b.z, ra * a.w + rb * b.w};
}

// The frame pair and blend of motion `mid` at time t.  t is used as given: outside [0, length] the phase clips to the first /
// last frame while the blend keeps following t, so the interpolation extrapolates exactly as the reference's does.
struct FrameBlend {
    int64_t f0, f1;
    float blend;
};
__device__ __forceinline__ FrameBlend motion_blend(const MotionClips& a, int mid, float t) {
    const float len = a.lengths[mid], dt = a.dt[mid];
    const int nf = a.num_frames[mid];
    const float phase = fminf(fmaxf(t / len, 0.f), 1.f);
    const int i0 = (int)(phase * (float)(nf - 1));
    const int i1 = min(i0 + 1, nf - 1);
    return FrameBlend{i0 + a.length_starts[mid], i1 + a.length_starts[mid], (t - (float)i0 * dt) / dt};
}
// world position of body b (amp_demo.hip keeps a key-body table longer than kMaxJoints)
__device__ __forceinline__ void motion_body(const MotionClips& a, const FrameBlend& fb, int b, float* out) {
    const float blend = fb.blend;
    const float* p0 = a.gts + fb.f0 * a.B * 3;
    const float* p1 = a.gts + fb.f1 * a.B * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = (1.f - blend) * p0[b * 3 + c] + blend * p1[b * 3 + c];
}
// world rotation of body b: the root rotation's expression (slerp of the frame pair's global rotations) on body b's rows
__device__ __forceinline__ void motion_body_rot(const MotionClips& a, const FrameBlend& fb, int b, float* out) {
    const Q4 rr = slerp(load_q(a.grs + (fb.f0 * a.B + b) * 4), load_q(a.grs + (fb.f1 * a.B + b) * 4), fb.blend);
    out[0] = rr.x; out[1] = rr.y; out[2] = rr.z; out[3] = rr.w;
}
// root position (lerp), rotation (slerp) and the two root velocities (unblended, frame 0 of the pair): body 0's pose
__device__ __forceinline__ void motion_root(const MotionClips& a, const FrameBlend& fb, float* root_pos, float* root_rot,
                                            float* root_vel, float* root_ang_vel) {
    motion_body(a, fb, 0, root_pos);
    motion_body_rot(a, fb, 0, root_rot);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        root_vel[c] = a.grvs[fb.f0 * 3 + c];
        root_ang_vel[c] = a.gravs[fb.f0 * 3 + c];
    }
}
// world position of key body k
__device__ __forceinline__ void motion_key(const MotionClips& a, const FrameBlend& fb, int k, float* out) {
    motion_body(a, fb, a.key_body[k], out);
}
// dof positions of joint j from its local rotation; dof d sits at dp[d * dof_stride]
__device__ __forceinline__ void motion_joint(const MotionClips& a, const FrameBlend& fb, int j, float* dp, int64_t dof_stride) {
    const int B = a.B;
    const int b = a.dof_body[j], o = a.dof_off[j], sz = a.dof_off[j + 1] - o;
    const Q4 q = slerp(load_q(a.lrs + (fb.f0 * B + b) * 4), load_q(a.lrs + (fb.f1 * B + b) * 4), fb.blend);
    // quaternion -> (angle, axis): below sin(theta/2) = 1e-5 (or NaN from w > 1) the rotation counts as none about z
    const float sn = sqrtf(1.f - q.w * q.w);
    float ang = 2.f * acosf(q.w);
    ang = atan2f(sinf(ang), cosf(ang));
    V3 ax{q.x / sn, q.y / sn, q.z / sn};
    if (!(fabsf(sn) > 1e-5f)) { ang = 0.f; ax = V3{0.f, 0.f, 1.f}; }
    if (sz == 3) {
        dp[o * dof_stride] = ang * ax.x; dp[(o + 1) * dof_stride] = ang * ax.y; dp[(o + 2) * dof_stride] = ang * ax.z;
    } else {
        const float th = ang * ax.y;                       // hinge joints turn about y
        dp[o * dof_stride] = atan2f(sinf(th), cosf(th));
    }
}
// The pose of motion `mid` at time t.  Dof element d of the two dof outputs sits at [d * dof_stride]; key_pos [K, 3].
__device__ __forceinline__ void motion_state_at(const MotionClips& a, int mid, float t, float* root_pos, float* root_rot,
                                                float* dp, float* root_vel, float* root_ang_vel, float* dof_vel,
                                                int64_t dof_stride, float* key_pos) {
    const FrameBlend fb = motion_blend(a, mid, t);
    motion_root(a, fb, root_pos, root_rot, root_vel, root_ang_vel);
    for (int k = 0; k < a.K; ++k) motion_key(a, fb, k, key_pos + 3 * k);
    for (int j = 0; j < a.J; ++j) motion_joint(a, fb, j, dp, dof_stride);
    for (int d = 0; d < a.D; ++d) dof_vel[d * dof_stride] = a.dvs[fb.f0 * a.D + d];
}

// the character's frame layout: J joints over D dofs, K key bodies
struct FrameDims {
    int D, K, J, local_root, root_height;
};

// One observation frame o[13 + 6 J + D + 3 K] in its parts.  Root columns o[0 .. 13); returns the inverse heading rotation:
__device__ __forceinline__ Q4 frame_root(const FrameDims& a, const float* rp, const float* rq, const float* v, const float* w,
                                           float* o) {
    const Q4 q{rq[0], rq[1], rq[2], rq[3]};
    const Q4 hq = heading_quat_inv(q);
    o[0] = a.root_height ? rp[2] : 0.f;
    tan_norm(a.local_root ? mul(hq, q) : q, o + 1);
    const V3 lv = rot(hq, V3{v[0], v[1], v[2]}), lw = rot(hq, V3{w[0], w[1], w[2]});
    o[7] = lv.x; o[8] = lv.y; o[9] = lv.z; o[10] = lw.x; o[11] = lw.y; o[12] = lw.z;
    return hq;
}
// the six columns of joint j (o: the frame): tangent + normal of its rotation
__device__ __forceinline__ void frame_joint(const int* dof_off, int j, const float* dp, int64_t dof_stride, float* o) {
    const int b = dof_off[j], sz = dof_off[j + 1] - b;
    Q4 jq;
    if (sz == 3) {                               // exponential map -> quaternion
        const V3 e{dp[b * dof_stride], dp[(b + 1) * dof_stride], dp[(b + 2) * dof_stride]};
        const float len = sqrtf(e.x * e.x + e.y * e.y + e.z * e.z);
        float ang = atan2f(sinf(len), cosf(len));
        V3 ax{e.x / len, e.y / len, e.z / len};
        if (!(fabsf(ang) > 1e-5f)) { ang = 0.f; ax = V3{0.f, 0.f, 1.f}; }
        jq = from_angle_axis(ang, ax);
    } else {                                     // hinge about y
        jq = from_angle_axis(dp[b * dof_stride], V3{0.f, 1.f, 0.f});
    }
    tan_norm(jq, o + 13 + 6 * j);
}
// heading-local position of a key body at kp (three world coordinates) -> out[3]; hq = heading_quat_inv(root rotation)
__device__ __forceinline__ void frame_key(const Q4& hq, const float* rp, const float* kp, float* out) {
    const V3 l = rot(hq, V3{kp[0] - rp[0], kp[1] - rp[1], kp[2] - rp[2]});
    out[0] = l.x; out[1] = l.y; out[2] = l.z;
}
// The whole frame from a root state, dof state (element d at [d * dof_stride]) and key body positions (key(k): pointer to
// the three world coordinates of key body k).
template <typename KeyPos>
__device__ __forceinline__ void amp_frame(const FrameDims& a, const int* dof_off, const float* rp, const float* rq,
                                          const float* v, const float* w, const float* dp, const float* dv,
                                          int64_t dof_stride, KeyPos key, float* o) {
    const Q4 hq = frame_root(a, rp, rq, v, w, o);
    for (int j = 0; j < a.J; ++j) frame_joint(dof_off, j, dp, dof_stride, o);
    const int od = 13 + 6 * a.J;
    for (int i = 0; i < a.D; ++i) o[od + i] = dv[i * dof_stride];
    for (int k = 0; k < a.K; ++k) frame_key(hq, rp, key(k), o + od + a.D + 3 * k);
}

}  // namespace
