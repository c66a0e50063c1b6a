// Quaternion helpers of the observation-side kernels (amp_obs.hip, env_obs.hip): xyzw, Hamilton product, written out the way
// the reference's tensor code evaluates them (isaacgym.torch_utils quat_rotate / quat_from_angle_axis, utils/torch_utils.py:
// 47-59 quat_to_tan_norm, 118-154 calc_heading / calc_heading_quat / calc_heading_quat_inv).  Both files compile with
// -ffp-contract=off, so every expression below rounds operation by operation.
#pragma once
#include "common.h"

namespace {

struct V3 { float x, y, z; };
struct Q4 { float x, y, z, w; };

// v rotated by the unit quaternion q (xyzw):  v (2 w^2 - 1) + 2 w (u x v) + 2 u (u . v)
__device__ __forceinline__ V3 rot(const Q4& q, const V3& v) {
    const float a = 2.f * q.w * q.w - 1.f, d = 2.f * (q.x * v.x + q.y * v.y + q.z * v.z), w2 = 2.f * q.w;
    return V3{v.x * a + (q.y * v.z - q.z * v.y) * w2 + q.x * d,
              v.y * a + (q.z * v.x - q.x * v.z) * w2 + q.y * d,
              v.z * a + (q.x * v.y - q.y * v.x) * w2 + q.z * d};
}
__device__ __forceinline__ Q4 mul(const Q4& a, const Q4& b) {
    return Q4{a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x,
              a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}
__device__ __forceinline__ Q4 from_angle_axis(float angle, V3 ax) {
    const float n = fmaxf(sqrtf(ax.x * ax.x + ax.y * ax.y + ax.z * ax.z), 1e-9f);
    const float s = sinf(0.5f * angle) / n, c = cosf(0.5f * angle);
    Q4 q{ax.x * s, ax.y * s, ax.z * s, c};
    const float m = fmaxf(sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w), 1e-9f);
    return Q4{q.x / m, q.y / m, q.z / m, q.w / m};
}
// tangent (rotated x axis) and normal (rotated z axis)
__device__ __forceinline__ void tan_norm(const Q4& q, float* o) {
    const V3 t = rot(q, V3{1.f, 0.f, 0.f}), n = rot(q, V3{0.f, 0.f, 1.f});
    o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = n.x; o[4] = n.y; o[5] = n.z;
}
__device__ __forceinline__ Q4 load_q(const float* p) { return Q4{p[0], p[1], p[2], p[3]}; }
// heading of q: the angle about z of its rotated x axis (atan2(0, 0) = 0 when that axis is vertical)
__device__ __forceinline__ float heading(const Q4& q) {
    const V3 d = rot(q, V3{1.f, 0.f, 0.f});
    return atan2f(d.y, d.x);
}
__device__ __forceinline__ Q4 heading_quat(const Q4& q) { return from_angle_axis(heading(q), V3{0.f, 0.f, 1.f}); }
// the inverse heading rotation: takes world vectors into the character's heading frame
__device__ __forceinline__ Q4 heading_quat_inv(const Q4& q) { return from_angle_axis(-heading(q), V3{0.f, 0.f, 1.f}); }

// ---- f64, the clip loader (motion_load.hip): poselib/core/rotation3d.py term by term, left to right.  These are separate
// functions, not overloads of the f32 ones above: the loader's products follow poselib's term order, the observation side
// isaacgym's.
struct V3d { double x, y, z; };
struct Q4d { double x, y, z, w; };

// quat_mul (rotation3d.py:8-20)
__device__ __forceinline__ Q4d quat_mul(const Q4d& a, const Q4d& b) {
    const double w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
    const double x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
    const double y = a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z;
    const double z = a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x;
    return Q4d{x, y, z, w};
}
__device__ __forceinline__ Q4d quat_conj(const Q4d& q) { return Q4d{-q.x, -q.y, -q.z, q.w}; }
// quat_normalize = quat_unit(quat_pos(q)) (rotation3d.py:24-49,88-93): the whole quaternion changes sign when w < 0,
// then every component is divided by max(norm, 1e-9)
__device__ __forceinline__ Q4d quat_normalize(Q4d q) {
    if (q.w < 0.0) q = Q4d{-q.x, -q.y, -q.z, -q.w};
    const double n = fmax(sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w), 1e-9);
    return Q4d{q.x / n, q.y / n, q.z / n, q.w / n};
}
__device__ __forceinline__ Q4d quat_mul_norm(const Q4d& a, const Q4d& b) { return quat_normalize(quat_mul(a, b)); }
// quat_rotate (rotation3d.py:201-206): the imaginary part of r (v, 0) conj(r), both products written out in full
__device__ __forceinline__ V3d quat_rotate(const Q4d& r, const V3d& v) {
    const Q4d p = quat_mul(quat_mul(r, Q4d{v.x, v.y, v.z, 0.0}), quat_conj(r));
    return V3d{p.x, p.y, p.z};
}

}  // namespace
