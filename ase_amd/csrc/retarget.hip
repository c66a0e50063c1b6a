// Motion retargeting: a mocap clip on its own skeleton -> a SkeletonMotion of the humanoid, all frames of all
// clips of a call in a fixed number of launches.  Follows poselib's SkeletonState.retarget_to (skeleton3d.py:786-948, reached
// through SkeletonMotion.retarget_to_by_tpose :1345-1390), retarget_motion.py (trim :211-226, project_joints :24-175,
// grounding :231-240) and SkeletonMotion.from_skeleton_state (skeleton3d.py:1090-1120,1223-1246) of the reference: f64,
// operation by operation (the file compiles with -ffp-contract=off), f64 between the launches, rounded to f32 once at the
// final store.  Clips are concatenated along the frame axis with the loader's tables; no stencil, pairing or reduction
// crosses a clip boundary.
//
// Every skeleton table is read from DEVICE memory (a source skeleton has up to 64 bodies, more than kernel arguments hold).
// A tree table is int32 [B, ld]: column 0 the depth of body b (links to the root of its chain), columns 1 .. depth + 1 its
// chain, the root first and b last.  The host cannot see these tables, so every index read from one is range-checked in the
// kernel; an item whose tables do not describe it writes nothing.
#include "quat.h"

namespace {

constexpr int kMaxBodies = 64;
constexpr int kThreads = 256;
constexpr int kTaps = 8;                     // gaussian_filter1d(sigma=2): radius int(4 * 2 + 0.5)

// exp(-x^2 / 8) / sum, x = 0 .. 8 (scipy.ndimage._gaussian_kernel1d, sigma 2, f64)
__device__ const double kGauss[kTaps + 1] = {
    0.199474647864745, 0.17603575888479034, 0.12098748976534904, 0.06475993660472744, 0.026995957967298846,
    0.00876430436278587, 0.002215963172596555, 0.0004363490205067883, 6.691628957263553e-05};

struct Tree { const int32_t* tab; int B, ld; };
struct FrameMap {                            // output frame t -> clip c, frame f of it, source row src_first[c] + f
    const int32_t *clip_first, *clip_frames, *src_first, *frame_clip;
    int C, T, Tsrc;
};

__device__ __forceinline__ Q4d load_qd(const double* p) { return Q4d{p[0], p[1], p[2], p[3]}; }
__device__ __forceinline__ void store_qd(double* p, const Q4d& q) { p[0] = q.x; p[1] = q.y; p[2] = q.z; p[3] = q.w; }
__device__ __forceinline__ void store_qf(float* p, const Q4d& q) {
    p[0] = (float)q.x; p[1] = (float)q.y; p[2] = (float)q.z; p[3] = (float)q.w;
}
__device__ __forceinline__ bool map_frame(const FrameMap& m, int t, int& c, int& f, int& n, int64_t& src) {
    c = m.frame_clip[t];
    if (c < 0 || c >= m.C) return false;
    f = t - m.clip_first[c];
    n = m.clip_frames[c];
    src = (int64_t)m.src_first[c] + f;
    return f >= 0 && f < n && m.clip_first[c] >= 0 && (int64_t)m.clip_first[c] + n <= m.T && src >= 0 && src < m.Tsrc;
}
// depth of body b, or -1 when the table row does not fit
__device__ __forceinline__ int tree_depth(const Tree& tr, int b) {
    const int d = tr.tab[(int64_t)b * tr.ld];
    return d >= 0 && d + 1 < tr.ld ? d : -1;
}
__device__ __forceinline__ int tree_node(const Tree& tr, int b, int d) {
    const int k = tr.tab[(int64_t)b * tr.ld + 1 + d];
    return k >= 0 && k < tr.B ? k : -1;
}
// quat_from_angle_axis (rotation3d.py:118-138)
__device__ __forceinline__ Q4d quat_from_angle_axis(double angle, const V3d& ax) {
    const double th = angle / 2.0;
    const double n = fmax(sqrt(ax.x * ax.x + ax.y * ax.y + ax.z * ax.z), 1e-9);
    const double s = sin(th), c = cos(th);
    return quat_normalize(Q4d{ax.x / n * s, ax.y / n * s, ax.z / n * s, c});
}
// quat_angle_axis times the angle (rotation3d.py:226-235), as motion_load.hip
__device__ __forceinline__ V3d quat_rotvec(const Q4d& d) {
    const double s = 2.0 * (d.w * d.w) - 1.0;
    const double angle = acos(fmin(fmax(s, -1.0), 1.0));
    const double m = fmax(sqrt(d.x * d.x + d.y * d.y + d.z * d.z), 1e-9);
    return V3d{d.x / m * angle, d.y / m * angle, d.z / m * angle};
}
// SkeletonState.global_transformation of body b (skeleton3d.py:403-424): `lr` the frame's local rotations [B, 4], `lt` the
// tree's offsets, `root` the frame's root translation (the local translation of body 0)
__device__ __forceinline__ bool fk_body(const Tree& tr, int b, const double* lr, const float* lt, const V3d& root, Q4d& gr,
                                        V3d& gt) {
    const int depth = tree_depth(tr, b);
    if (depth < 0) return false;
    for (int d = 0; d <= depth; ++d) {
        const int k = tree_node(tr, b, d);
        if (k < 0) return false;
        const V3d l = k == 0 ? root : V3d{(double)lt[3 * k], (double)lt[3 * k + 1], (double)lt[3 * k + 2]};
        if (d == 0) {
            gr = load_qd(lr + 4 * k);
            gt = l;
        } else {                                             // transform_mul(global[parent], local[k])
            const V3d r = quat_rotate(gr, l);
            gt = V3d{r.x + gt.x, r.y + gt.y, r.z + gt.z};
            gr = quat_mul_norm(gr, load_qd(lr + 4 * k));
        }
    }
    return true;
}

// ---- 1. global rotations of a tree.  mode 0: forward kinematics of local rotations; 1: stored global rotations, as they
// are; 2: stored global rotations taken to local form on the tree first (SkeletonState.local_rotation :462-482), then
// forward kinematics - what a T-pose file in global form goes through
struct FkArgs { const double* rot; double* out; Tree tr; FrameMap m; int mode; };

__global__ __launch_bounds__(kThreads) void retarget_fk_kernel(FkArgs a) {
    const int B = a.tr.B;
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= (int64_t)a.m.T * B) return;
    const int t = (int)(idx / B), b = (int)(idx - (int64_t)t * B);
    int c, f, n; int64_t src;
    if (!map_frame(a.m, t, c, f, n, src)) return;
    const double* q = a.rot + src * B * 4;
    Q4d g = load_qd(q + 4 * b);
    if (a.mode != 1) {
        const int depth = tree_depth(a.tr, b);
        if (depth < 0) return;
        int prev = -1;
        for (int d = 0; d <= depth; ++d) {
            const int k = tree_node(a.tr, b, d);
            if (k < 0) return;
            Q4d l = load_qd(q + 4 * k);
            if (a.mode == 2 && d > 0) l = quat_mul_norm(quat_conj(load_qd(q + 4 * prev)), l);
            g = d == 0 ? l : quat_mul_norm(g, l);
            prev = k;
        }
    }
    store_qd(a.out + ((int64_t)t * B + b) * 4, g);
}

// ---- 2. the reduced trees (_transfer_to :706-713, _remapped_to :757-784, STEP 2 :881-903): source global rotations -> local
// on the reduced SOURCE tree -> recomposed along the reduced TARGET tree, node 0 pre-multiplied by the rotation to the target
struct ChainArgs {
    const double* gs;                        // [T, Bs, 4]
    double* out;                             // [T, M, 4]
    const int32_t *rs_body, *rs_parent, *rt_src;      // [M]: source body / reduced-source parent of a reduced-source node; reduced-source node of a reduced-target node
    const double* params;                    // [0..3] the rotation to the target skeleton
    Tree rt;                                 // the reduced target tree
    int T, Bs;
};

__device__ __forceinline__ bool reduced_local(const ChainArgs& a, const double* g, int k, Q4d& l) {
    const int M = a.rt.B;
    const int m = a.rt_src[k];
    if (m < 0 || m >= M) return false;
    const int body = a.rs_body[m], p = a.rs_parent[m];
    if (body < 0 || body >= a.Bs || p < -1 || p >= M) return false;
    l = load_qd(g + 4 * body);
    if (p >= 0) {
        const int pb = a.rs_body[p];
        if (pb < 0 || pb >= a.Bs) return false;
        l = quat_mul_norm(quat_conj(load_qd(g + 4 * pb)), l);
    }
    if (k == 0) l = quat_mul_norm(load_qd(a.params), l);
    return true;
}

__global__ __launch_bounds__(kThreads) void retarget_chain_kernel(ChainArgs a) {
    const int M = a.rt.B;
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= (int64_t)a.T * M) return;
    const int t = (int)(idx / M), i = (int)(idx - (int64_t)t * M);
    const double* g = a.gs + (int64_t)t * a.Bs * 4;
    const int depth = tree_depth(a.rt, i);
    if (depth < 0) return;
    Q4d gr{0.0, 0.0, 0.0, 1.0};
    for (int d = 0; d <= depth; ++d) {
        const int k = tree_node(a.rt, i, d);
        Q4d l;
        if (k < 0 || !reduced_local(a, g, k, l)) return;
        gr = d == 0 ? l : quat_mul_norm(gr, l);
    }
    store_qd(a.out + ((int64_t)t * M + i) * 4, gr);
}

// ---- 3. STEP 3-5 (:905-946): the rotation relative to the source T-pose re-applied to the target T-pose, spread over the
// full target tree (a body outside the mapping takes its nearest mapped ancestor's), local_repr on it; the root translation
struct PoseArgs {
    const double *g_state, *g_tpose, *g_target;      // [T, M, 4] [M, 4] [Bt, 4]
    const double* root_t;                            // [Tsrc, 3]
    const double* params;                            // R [4], source T-pose root [3], target T-pose root [3], scale
    const int32_t *rt_body, *anc, *parent;           // [M] target body of a reduced-target node; [Bt] reduced-target node a body takes; [Bt]
    double *lr, *rt;                                 // [T, Bt, 4] [T, 3]
    FrameMap m;
    int M, Bt;
};

__device__ __forceinline__ bool new_global(const PoseArgs& a, int t, int body, Q4d& g) {
    const int i = a.anc[body];
    if (i < 0 || i >= a.M) return false;
    const int tb = a.rt_body[i];
    if (tb < 0 || tb >= a.Bt) return false;
    const Q4d diff = quat_mul_norm(load_qd(a.g_state + ((int64_t)t * a.M + i) * 4), quat_conj(load_qd(a.g_tpose + 4 * i)));
    g = quat_mul_norm(diff, load_qd(a.g_target + 4 * tb));
    return true;
}

__global__ __launch_bounds__(kThreads) void retarget_pose_kernel(PoseArgs a) {
    const int B = a.Bt;
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= (int64_t)a.m.T * B) return;
    const int t = (int)(idx / B), b = (int)(idx - (int64_t)t * B);
    int c, f, n; int64_t src;
    if (!map_frame(a.m, t, c, f, n, src)) return;
    const int p = a.parent[b];
    Q4d g, gp;
    if (p < -1 || p >= B || !new_global(a, t, b, g) || (p >= 0 && !new_global(a, t, p, gp))) return;
    store_qd(a.lr + ((int64_t)t * B + b) * 4, p < 0 ? g : quat_mul_norm(quat_conj(gp), g));
    if (b == 0) {
        const Q4d R = load_qd(a.params);
        const V3d s = quat_rotate(R, V3d{a.root_t[3 * src], a.root_t[3 * src + 1], a.root_t[3 * src + 2]});
        const V3d s0 = quat_rotate(R, V3d{a.params[4], a.params[5], a.params[6]});
        const double scale = a.params[10];
        a.rt[3 * (int64_t)t] = a.params[7] + (s.x - s0.x) * scale;
        a.rt[3 * (int64_t)t + 1] = a.params[8] + (s.y - s0.y) * scale;
        a.rt[3 * (int64_t)t + 2] = a.params[9] + (s.z - s0.z) * scale;
    }
}

// ---- 4. project_joints (retarget_motion.py:24-175) from a table: a body is copied (role 0), set to identity (1), the upper
// (2) or the lower (3) body of a limb row (upper, lower, end, bend sign, twist sense).  Every limb reads the UNPROJECTED motion.
struct HingeArgs {
    const double *lr, *rt;                   // [T, B, 4] [T, 3]
    const float* lt;                         // [B, 3]
    const int32_t* roles;                    // [B, 6]: role, upper, lower, end, bend sign (+-1), twist sense (+-1)
    double* out;                             // [T, B, 4]
    Tree tr;
    int T;
};

__global__ __launch_bounds__(kThreads) void retarget_hinge_kernel(HingeArgs a) {
    const int B = a.tr.B;
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= (int64_t)a.T * B) return;
    const int t = (int)(idx / B), b = (int)(idx - (int64_t)t * B);
    const double* lr = a.lr + (int64_t)t * B * 4;
    double* o = a.out + ((int64_t)t * B + b) * 4;
    const int32_t* r = a.roles + 6 * b;
    const int role = r[0];
    if (role == 0) { store_qd(o, load_qd(lr + 4 * b)); return; }
    if (role == 1) { store_qd(o, Q4d{0.0, 0.0, 0.0, 1.0}); return; }
    const int u = r[1], l = r[2], e = r[3];
    if ((role != 2 && role != 3) || u < 0 || u >= B || l < 0 || l >= B || e < 0 || e >= B) return;
    const V3d root{a.rt[3 * (int64_t)t], a.rt[3 * (int64_t)t + 1], a.rt[3 * (int64_t)t + 2]};
    Q4d gq; V3d pu, pl, pe;
    if (!fk_body(a.tr, u, lr, a.lt, root, gq, pu) || !fk_body(a.tr, l, lr, a.lt, root, gq, pl) ||
        !fk_body(a.tr, e, lr, a.lt, root, gq, pe)) return;
    V3d d0{pu.x - pl.x, pu.y - pl.y, pu.z - pl.z}, d1{pe.x - pl.x, pe.y - pl.y, pe.z - pl.z};
    const double n0 = sqrt(d0.x * d0.x + d0.y * d0.y + d0.z * d0.z), n1 = sqrt(d1.x * d1.x + d1.y * d1.y + d1.z * d1.z);
    d0 = V3d{d0.x / n0, d0.y / n0, d0.z / n0};
    d1 = V3d{d1.x / n1, d1.y / n1, d1.z / n1};
    const double dot = -d0.x * d1.x + -d0.y * d1.y + -d0.z * d1.z;
    const double theta = acos(fmin(fmax(dot, -1.0), 1.0));
    const Q4d bend = quat_from_angle_axis(r[4] < 0 ? -fabs(theta) : fabs(theta), V3d{0.0, 1.0, 0.0});
    if (role == 3) { store_qd(o, bend); return; }
    V3d dir{(double)a.lt[3 * e], (double)a.lt[3 * e + 1], (double)a.lt[3 * e + 2]};
    const double nd = sqrt(dir.x * dir.x + dir.y * dir.y + dir.z * dir.z);
    dir = V3d{dir.x / nd, dir.y / nd, dir.z / nd};
    const V3d dir0 = quat_rotate(load_qd(lr + 4 * l), dir), dir1 = quat_rotate(bend, dir);
    const double tdot = dir0.x * dir1.x + dir0.y * dir1.y + dir0.z * dir1.z;
    double twist = acos(fmin(fmax(tdot, -1.0), 1.0));
    if (!(r[5] < 0 ? dir0.y <= 0.0 : dir0.y >= 0.0)) twist = -twist;
    store_qd(o, quat_mul(load_qd(lr + 4 * u), quat_from_angle_axis(twist, dir)));
}

// ---- 5. grounding (retarget_motion.py:231-236): per clip the minimum of global z over its frames and bodies.  One block per
// clip; the order of the comparisons is fixed and a minimum does not depend on it anyway.  A NaN wins, as torch.min.
struct GroundArgs {
    const double *lr, *rt;
    const float* lt;
    const int32_t *clip_first, *clip_frames;
    double* min_z;                           // [C]
    Tree tr;
    int T;
};

__device__ __forceinline__ double min_nan(double m, double v) { return (v < m || v != v) && m == m ? v : m; }

__global__ __launch_bounds__(kThreads) void retarget_ground_kernel(GroundArgs a) {
    __shared__ double red[kThreads];
    const int B = a.tr.B, c = blockIdx.x;
    const int first = a.clip_first[c], n = a.clip_frames[c];
    double m = INFINITY;
    if (first >= 0 && n >= 0 && (int64_t)first + n <= a.T) {
        for (int64_t i = threadIdx.x; i < (int64_t)n * B; i += kThreads) {
            const int64_t t = first + i / B;
            const int b = (int)(i % B);
            Q4d gq; V3d gt;
            if (fk_body(a.tr, b, a.lr + t * B * 4, a.lt, V3d{a.rt[3 * t], a.rt[3 * t + 1], a.rt[3 * t + 2]}, gq, gt))
                m = min_nan(m, gt.z);
        }
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = min_nan(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) a.min_z[c] = red[0];
}

// ---- 6. the grounded motion (retarget_motion.py:236-243): root z += -min, += the height offset; its global transforms in
// f64 for the velocities; the clip's local rotations and root translation rounded to f32
struct FinishArgs {
    const double *lr, *rt, *min_z, *params;  // params[11]: root height offset
    const float* lt;
    const int32_t* frame_clip;
    double *gr, *gt;                         // [T, B, 4] [T, B, 3]
    float *rot_out, *root_out;               // [T, B, 4] [T, 3]
    Tree tr;
    int T, C;
};

__global__ __launch_bounds__(kThreads) void retarget_finish_kernel(FinishArgs a) {
    const int B = a.tr.B;
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= (int64_t)a.T * B) return;
    const int t = (int)(idx / B), b = (int)(idx - (int64_t)t * B);
    const int c = a.frame_clip[t];
    if (c < 0 || c >= a.C) return;
    const double* lr = a.lr + (int64_t)t * B * 4;
    const V3d root{a.rt[3 * (int64_t)t], a.rt[3 * (int64_t)t + 1], a.rt[3 * (int64_t)t + 2] + -a.min_z[c] + a.params[11]};
    Q4d gr; V3d gt;
    if (!fk_body(a.tr, b, lr, a.lt, root, gr, gt)) return;
    const int64_t o = (int64_t)t * B + b;
    store_qd(a.gr + o * 4, gr);
    a.gt[o * 3] = gt.x; a.gt[o * 3 + 1] = gt.y; a.gt[o * 3 + 2] = gt.z;
    store_qf(a.rot_out + o * 4, load_qd(lr + 4 * b));
    if (b == 0) {
        a.root_out[3 * (int64_t)t] = (float)root.x; a.root_out[3 * (int64_t)t + 1] = (float)root.y;
        a.root_out[3 * (int64_t)t + 2] = (float)root.z;
    }
}

// ---- 7. SkeletonMotion._compute_velocity / _compute_angular_velocity (skeleton3d.py:1223-1246).  numpy.gradient along the
// frames of the clip (central differences, one-sided ends), scipy's gaussian_filter1d(sigma=2, mode='nearest') in the order
// its symmetric correlation adds (centre tap, then the pairs from the outermost in), indices clamped to the clip.
struct VelArgs {
    const double *gr, *gt, *clip_fps;
    const int32_t *clip_first, *clip_frames, *frame_clip;
    float *vel, *ang;                        // [T, B, 3]
    int T, C, B;
};

__device__ __forceinline__ V3d grad_at(const double* p, int64_t stride, int j, int n) {   // p: frame 0 of the clip, this body
    if (j == 0 || j == n - 1) {
        const double* a = p + (int64_t)(j == 0 ? 0 : n - 2) * stride;
        const double* b = a + stride;
        return V3d{(b[0] - a[0]) / 1.0, (b[1] - a[1]) / 1.0, (b[2] - a[2]) / 1.0};
    }
    const double *a = p + (int64_t)(j - 1) * stride, *b = p + (int64_t)(j + 1) * stride;
    return V3d{(b[0] - a[0]) / 2.0, (b[1] - a[1]) / 2.0, (b[2] - a[2]) / 2.0};
}
__device__ __forceinline__ V3d angvel_at(const double* q, int64_t stride, int j, int n, double dt) {
    if (j == n - 1) return V3d{0.0, 0.0, 0.0};               // the identity's angle is acos(1) = 0
    const Q4d d = quat_mul_norm(load_qd(q + (int64_t)(j + 1) * stride), quat_conj(load_qd(q + (int64_t)j * stride)));
    const V3d v = quat_rotvec(d);
    return V3d{v.x / dt, v.y / dt, v.z / dt};
}
__device__ __forceinline__ int clampi(int x, int hi) { return x < 0 ? 0 : (x > hi ? hi : x); }

__global__ __launch_bounds__(kThreads) void retarget_vel_kernel(VelArgs a) {
    const int B = a.B;
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= (int64_t)a.T * B) return;
    const int t = (int)(idx / B), b = (int)(idx - (int64_t)t * B);
    const int c = a.frame_clip[t];
    if (c < 0 || c >= a.C) return;
    const int first = a.clip_first[c], n = a.clip_frames[c], f = t - first;
    if (first < 0 || n < 2 || (int64_t)first + n > a.T || f < 0 || f >= n) return;
    const double dt = 1.0 / a.clip_fps[c];
    const double* p = a.gt + ((int64_t)first * B + b) * 3;
    const double* q = a.gr + ((int64_t)first * B + b) * 4;
    const V3d g0 = grad_at(p, (int64_t)B * 3, f, n), w0 = angvel_at(q, (int64_t)B * 4, f, n, dt);
    V3d v{g0.x * kGauss[0], g0.y * kGauss[0], g0.z * kGauss[0]}, w{w0.x * kGauss[0], w0.y * kGauss[0], w0.z * kGauss[0]};
    for (int k = kTaps; k >= 1; --k) {
        const int lo = clampi(f - k, n - 1), hi = clampi(f + k, n - 1);
        const V3d ga = grad_at(p, (int64_t)B * 3, lo, n), gb = grad_at(p, (int64_t)B * 3, hi, n);
        const V3d wa = angvel_at(q, (int64_t)B * 4, lo, n, dt), wb = angvel_at(q, (int64_t)B * 4, hi, n, dt);
        const double g = kGauss[k];
        v = V3d{v.x + (ga.x + gb.x) * g, v.y + (ga.y + gb.y) * g, v.z + (ga.z + gb.z) * g};
        w = V3d{w.x + (wa.x + wb.x) * g, w.y + (wa.y + wb.y) * g, w.z + (wa.z + wb.z) * g};
    }
    const int64_t o = ((int64_t)t * B + b) * 3;
    a.vel[o] = (float)(v.x / dt); a.vel[o + 1] = (float)(v.y / dt); a.vel[o + 2] = (float)(v.z / dt);
    a.ang[o] = (float)w.x; a.ang[o + 1] = (float)w.y; a.ang[o + 2] = (float)w.z;
}

inline unsigned blocks_for(int64_t items) { return (unsigned)((items + kThreads - 1) / kThreads); }

}  // namespace

#define RT_CHECK_SIZES(name, T, B)                                                                                   \
    ASE_CHECK_ARG((B) >= 1 && (B) <= kMaxBodies, name ": %d bodies (1-%d)", (int)(B), kMaxBodies);                 \
    ASE_CHECK_ARG((T) >= 1 && (int64_t)(T) * (B) < (int64_t)1 << 31, name ": %d frames (1 or more, frames x bodies below 2^31)", (int)(T))
#define RT_CHECK_MAP(name)                                                                                           \
    ASE_CHECK_ARG(n_clips >= 1 && n_clips <= n_frames && n_src_frames >= n_frames, name ": bad sizes (%d clips, %d frames of %d source frames)", \
                  n_clips, n_frames, n_src_frames)

extern "C" int ase_hip_retarget_fk(const double* rotation, int mode, const int32_t* tree, int tree_ld, int n_bodies,
                                   const int32_t* clip_first, const int32_t* clip_num_frames, const int32_t* src_first,
                                   const int32_t* frame_clip, int n_clips, int n_frames, int n_src_frames, double* out,
                                   void* stream) {
    ASE_CHECK_ARG(rotation && tree && clip_first && clip_num_frames && src_first && frame_clip && out, "retarget_fk: null operand");
    ASE_CHECK_ARG(mode >= 0 && mode <= 2, "retarget_fk: mode %d (0 local, 1 global, 2 global through local)", mode);
    RT_CHECK_SIZES("retarget_fk", n_frames, n_bodies);
    RT_CHECK_MAP("retarget_fk");
    ASE_CHECK_ARG(tree_ld >= 2 && tree_ld <= kMaxBodies + 1, "retarget_fk: tree table of %d columns (2-%d)", tree_ld, kMaxBodies + 1);
    FkArgs a{rotation, out, Tree{tree, n_bodies, tree_ld},
             FrameMap{clip_first, clip_num_frames, src_first, frame_clip, n_clips, n_frames, n_src_frames}, mode};
    ASE_LAUNCH(retarget_fk_kernel, dim3(blocks_for((int64_t)n_frames * n_bodies)), dim3(kThreads), 0, (hipStream_t)stream, a);
    ASE_CHECK_LAUNCH("retarget_fk");
    return ASE_OK;
}

extern "C" int ase_hip_retarget_chain(const double* src_global, int n_src_bodies, const int32_t* rs_body,
                                      const int32_t* rs_parent, const int32_t* rt_src, const int32_t* rt_tree, int tree_ld,
                                      int n_mapped, const double* params, int n_frames, double* out, void* stream) {
    ASE_CHECK_ARG(src_global && rs_body && rs_parent && rt_src && rt_tree && params && out, "retarget_chain: null operand");
    RT_CHECK_SIZES("retarget_chain", n_frames, n_src_bodies);
    ASE_CHECK_ARG(n_mapped >= 1 && n_mapped <= n_src_bodies, "retarget_chain: %d mapped bodies of %d", n_mapped, n_src_bodies);
    ASE_CHECK_ARG(tree_ld >= 2 && tree_ld <= kMaxBodies + 1, "retarget_chain: tree table of %d columns (2-%d)", tree_ld, kMaxBodies + 1);
    ChainArgs a{src_global, out, rs_body, rs_parent, rt_src, params, Tree{rt_tree, n_mapped, tree_ld}, n_frames, n_src_bodies};
    ASE_LAUNCH(retarget_chain_kernel, dim3(blocks_for((int64_t)n_frames * n_mapped)), dim3(kThreads), 0, (hipStream_t)stream, a);
    ASE_CHECK_LAUNCH("retarget_chain");
    return ASE_OK;
}

extern "C" int ase_hip_retarget_pose(const double* state_global, const double* tpose_global, const double* target_global,
                                     const double* root_translation, const double* params, const int32_t* rt_body,
                                     const int32_t* ancestor, const int32_t* parent_indices, int n_mapped, int n_bodies,
                                     const int32_t* clip_first, const int32_t* clip_num_frames, const int32_t* src_first,
                                     const int32_t* frame_clip, int n_clips, int n_frames, int n_src_frames,
                                     double* local_rotation, double* root_out, void* stream) {
    ASE_CHECK_ARG(state_global && tpose_global && target_global && root_translation && params && rt_body && ancestor &&
                      parent_indices && clip_first && clip_num_frames && src_first && frame_clip && local_rotation && root_out,
                  "retarget_pose: null operand");
    RT_CHECK_SIZES("retarget_pose", n_frames, n_bodies);
    RT_CHECK_MAP("retarget_pose");
    ASE_CHECK_ARG(n_mapped >= 1 && n_mapped <= n_bodies, "retarget_pose: %d mapped bodies of %d", n_mapped, n_bodies);
    PoseArgs a{state_global, tpose_global, target_global, root_translation, params, rt_body, ancestor, parent_indices,
               local_rotation, root_out,
               FrameMap{clip_first, clip_num_frames, src_first, frame_clip, n_clips, n_frames, n_src_frames}, n_mapped, n_bodies};
    ASE_LAUNCH(retarget_pose_kernel, dim3(blocks_for((int64_t)n_frames * n_bodies)), dim3(kThreads), 0, (hipStream_t)stream, a);
    ASE_CHECK_LAUNCH("retarget_pose");
    return ASE_OK;
}

extern "C" int ase_hip_retarget_hinge(const double* local_rotation, const double* root_translation,
                                      const float* local_translation, const int32_t* tree, int tree_ld, const int32_t* roles,
                                      int n_bodies, int n_frames, double* out, void* stream) {
    ASE_CHECK_ARG(local_rotation && root_translation && local_translation && tree && roles && out, "retarget_hinge: null operand");
    RT_CHECK_SIZES("retarget_hinge", n_frames, n_bodies);
    ASE_CHECK_ARG(tree_ld >= 2 && tree_ld <= kMaxBodies + 1, "retarget_hinge: tree table of %d columns (2-%d)", tree_ld, kMaxBodies + 1);
    HingeArgs a{local_rotation, root_translation, local_translation, roles, out, Tree{tree, n_bodies, tree_ld}, n_frames};
    ASE_LAUNCH(retarget_hinge_kernel, dim3(blocks_for((int64_t)n_frames * n_bodies)), dim3(kThreads), 0, (hipStream_t)stream, a);
    ASE_CHECK_LAUNCH("retarget_hinge");
    return ASE_OK;
}

extern "C" int ase_hip_retarget_ground(const double* local_rotation, const double* root_translation,
                                       const float* local_translation, const int32_t* tree, int tree_ld, int n_bodies,
                                       const int32_t* clip_first, const int32_t* clip_num_frames, int n_clips, int n_frames,
                                       double* min_z, void* stream) {
    ASE_CHECK_ARG(local_rotation && root_translation && local_translation && tree && clip_first && clip_num_frames && min_z,
                  "retarget_ground: null operand");
    RT_CHECK_SIZES("retarget_ground", n_frames, n_bodies);
    ASE_CHECK_ARG(n_clips >= 1 && n_clips <= n_frames, "retarget_ground: bad sizes (%d clips, %d frames)", n_clips, n_frames);
    ASE_CHECK_ARG(tree_ld >= 2 && tree_ld <= kMaxBodies + 1, "retarget_ground: tree table of %d columns (2-%d)", tree_ld, kMaxBodies + 1);
    GroundArgs a{local_rotation, root_translation, local_translation, clip_first, clip_num_frames, min_z,
                 Tree{tree, n_bodies, tree_ld}, n_frames};
    ASE_LAUNCH(retarget_ground_kernel, dim3((unsigned)n_clips), dim3(kThreads), 0, (hipStream_t)stream, a);
    ASE_CHECK_LAUNCH("retarget_ground");
    return ASE_OK;
}

extern "C" int ase_hip_retarget_finish(const double* local_rotation, const double* root_translation, const double* min_z,
                                       const double* params, const float* local_translation, const int32_t* tree, int tree_ld,
                                       int n_bodies, const int32_t* frame_clip, int n_clips, int n_frames,
                                       double* global_rotation, double* global_translation, float* rotation_out,
                                       float* root_out, void* stream) {
    ASE_CHECK_ARG(local_rotation && root_translation && min_z && params && local_translation && tree && frame_clip &&
                      global_rotation && global_translation && rotation_out && root_out, "retarget_finish: null operand");
    RT_CHECK_SIZES("retarget_finish", n_frames, n_bodies);
    ASE_CHECK_ARG(n_clips >= 1 && n_clips <= n_frames, "retarget_finish: bad sizes (%d clips, %d frames)", n_clips, n_frames);
    ASE_CHECK_ARG(tree_ld >= 2 && tree_ld <= kMaxBodies + 1, "retarget_finish: tree table of %d columns (2-%d)", tree_ld, kMaxBodies + 1);
    FinishArgs a{local_rotation, root_translation, min_z, params, local_translation, frame_clip, global_rotation,
                 global_translation, rotation_out, root_out, Tree{tree, n_bodies, tree_ld}, n_frames, n_clips};
    ASE_LAUNCH(retarget_finish_kernel, dim3(blocks_for((int64_t)n_frames * n_bodies)), dim3(kThreads), 0, (hipStream_t)stream, a);
    ASE_CHECK_LAUNCH("retarget_finish");
    return ASE_OK;
}

extern "C" int ase_hip_retarget_velocity(const double* global_rotation, const double* global_translation, int n_bodies,
                                         const int32_t* clip_first, const int32_t* clip_num_frames, const double* clip_fps,
                                         const int32_t* frame_clip, int n_clips, int n_frames, float* velocity,
                                         float* angular_velocity, void* stream) {
    ASE_CHECK_ARG(global_rotation && global_translation && clip_first && clip_num_frames && clip_fps && frame_clip && velocity &&
                      angular_velocity, "retarget_velocity: null operand");
    RT_CHECK_SIZES("retarget_velocity", n_frames, n_bodies);
    ASE_CHECK_ARG(n_clips >= 1 && n_frames >= 2 * (int64_t)n_clips, "retarget_velocity: bad sizes (%d clips, %d frames; a clip has 2 or more)",
                  n_clips, n_frames);
    VelArgs a{global_rotation, global_translation, clip_fps, clip_first, clip_num_frames, frame_clip, velocity, angular_velocity,
              n_frames, n_clips, n_bodies};
    ASE_LAUNCH(retarget_vel_kernel, dim3(blocks_for((int64_t)n_frames * n_bodies)), dim3(kThreads), 0, (hipStream_t)stream, a);
    ASE_CHECK_LAUNCH("retarget_velocity");
    return ASE_OK;
}
