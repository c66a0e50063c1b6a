// Motion-clip loader: the frame arrays ase_hip_motion_state / ase_hip_amp_reset read (gts, grs, lrs, grvs,
// gravs, dvs) from the raw contents of SkeletonMotion clip files, all frames of all clips in ONE launch.  Follows
// MotionLib._load_motions / _compute_motion_dof_vels (utils/motion_lib.py:75-80,279-294,326-355) and poselib's forward
// kinematics (SkeletonState.global_transformation, skeleton3d.py:403-424,495-510) of the reference: f64, operation by
// operation (the file compiles with -ffp-contract=off), rounded to f32 once at the store.
#include "quat.h"

namespace {

constexpr int kMaxClipBodies = 32;          // bodies of a skeleton: the ancestor table below lives in the kernel arguments
constexpr int kMaxClipJoints = 32;
constexpr int kThreads = 256;

struct ClipFramesArgs {
    const double *rot, *root_t, *root_v, *root_w;            // [T, B, 4] [T, 3] x3
    const float* local_t;                                    // [C, B, 3]
    const int32_t *clip_first, *clip_frames, *frame_clip;    // [C] [C] [T]
    const double* clip_fps;                                  // [C]
    float *gts, *grs, *lrs, *grvs, *gravs, *dvs;
    int T, C, B, J, D;
    int dof_off[kMaxClipJoints + 1];
    uint8_t dof_body[kMaxClipJoints];
    uint8_t depth[kMaxClipBodies];                           // links between a body and the root of its chain
    uint8_t chain[kMaxClipBodies][kMaxClipBodies];           // chain[b][0 .. depth[b]]: the root first, b last
};

__device__ __forceinline__ Q4d load_qd(const double* p) { return Q4d{p[0], p[1], p[2], p[3]}; }
__device__ __forceinline__ void store_q(float* p, const Q4d& q) {
    p[0] = (float)q.x; p[1] = (float)q.y; p[2] = (float)q.z; p[3] = (float)q.w;
}

// One thread per (frame, item): items 0 .. B-1 are the bodies (forward kinematics), items B .. B+J-1 the joints (velocities).
// A body walks its own ancestor chain from the root down - the operations and their order are those of the reference's
// loop over the bodies in index order, which reuses the parent's result; recomputing it costs at most depth x 60 flops and
// needs no storage or synchronisation (a thread per frame would hold every body's transform, indexed by a run-time parent id).
__global__ __launch_bounds__(kThreads) void clip_frames_kernel(ClipFramesArgs a) {
    const int B = a.B, W = a.B + a.J;
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= (int64_t)a.T * W) return;
    const int t = (int)(idx / W), item = (int)(idx - (int64_t)t * W);
    const int c = a.frame_clip[t];
    if (c < 0 || c >= a.C) return;                           // a frame of no clip: nothing is read or written for it
    const double* q = a.rot + (int64_t)t * B * 4;
    if (item < B) {
        const int b = item;
        const float* lt = a.local_t + (int64_t)c * B * 3;
        const int64_t o = (int64_t)t * B + b;
        store_q(a.lrs + o * 4, load_qd(q + 4 * b));
        // the root of the chain: its global transform is its local one, the stored rotation as it is.  Body 0's translation
        // is the clip's root translation ROUNDED TO F32 (poselib writes it into the tree's f32 local_translation tensor)
        const int k0 = a.chain[b][0];
        Q4d gr = load_qd(q + 4 * k0);
        V3d gt = k0 == 0 ? V3d{(double)(float)a.root_t[3 * (int64_t)t], (double)(float)a.root_t[3 * (int64_t)t + 1],
                               (double)(float)a.root_t[3 * (int64_t)t + 2]}
                         : V3d{(double)lt[3 * k0], (double)lt[3 * k0 + 1], (double)lt[3 * k0 + 2]};
        const int depth = a.depth[b];
        for (int d = 1; d <= depth; ++d) {                   // transform_mul(global[parent], local[k]) (rotation3d.py:318-327)
            const int k = a.chain[b][d];
            const V3d r = quat_rotate(gr, V3d{(double)lt[3 * k], (double)lt[3 * k + 1], (double)lt[3 * k + 2]});
            gt = V3d{r.x + gt.x, r.y + gt.y, r.z + gt.z};
            gr = quat_mul_norm(gr, load_qd(q + 4 * k));
        }
        store_q(a.grs + o * 4, gr);
        a.gts[o * 3] = (float)gt.x; a.gts[o * 3 + 1] = (float)gt.y; a.gts[o * 3 + 2] = (float)gt.z;
        if (b == 0) {
            for (int x = 0; x < 3; ++x) {
                a.grvs[3 * (int64_t)t + x] = (float)a.root_v[3 * (int64_t)t + x];
                a.gravs[3 * (int64_t)t + x] = (float)a.root_w[3 * (int64_t)t + x];
            }
        }
        return;
    }
    // joint velocities (_local_rotation_to_dof_vel): frame f of its clip pairs with f + 1, the last frame repeats the pair
    // before it; frames of different clips never pair
    const int j = item - B;
    const int off = a.dof_off[j], size = a.dof_off[j + 1] - off;
    float* dv = a.dvs + (int64_t)t * a.D + off;
    const int f = t - a.clip_first[c], n = a.clip_frames[c];
    const int t0 = f < n - 1 ? t : t - 1;
    if (f < 0 || f >= n || n < 2 || t0 < 0 || t0 + 1 >= a.T) {          // tables that do not describe the frames: zeros
        for (int x = 0; x < size; ++x) dv[x] = 0.f;
        return;
    }
    const int b = a.dof_body[j];
    const double dt = 1.0 / a.clip_fps[c];
    const double* q0 = a.rot + ((int64_t)t0 * B + b) * 4;
    const Q4d d = quat_mul_norm(quat_conj(load_qd(q0)), load_qd(q0 + (int64_t)B * 4));
    // quat_angle_axis (rotation3d.py:226-235): the reference's formula, ill-conditioned near the identity as it is
    const double s = 2.0 * (d.w * d.w) - 1.0;
    const double angle = acos(fmin(fmax(s, -1.0), 1.0));
    const double m = fmax(sqrt(d.x * d.x + d.y * d.y + d.z * d.z), 1e-9);
    const V3d v{d.x / m * angle / dt, d.y / m * angle / dt, d.z / m * angle / dt};
    if (size == 3) {
        dv[0] = (float)v.x; dv[1] = (float)v.y; dv[2] = (float)v.z;
    } else {
        dv[0] = (float)v.y;                                  // a 1-dof joint turns about y
    }
}

}  // namespace

extern "C" int ase_hip_clip_frames(const double* rotation, const double* root_translation, const double* root_velocity,
                                   const double* root_angular_velocity, const float* local_translation,
                                   const int32_t* parent_indices, int n_bodies, const int32_t* clip_first,
                                   const int32_t* clip_num_frames, const double* clip_fps, const int32_t* frame_clip,
                                   int n_clips, int n_frames, const int32_t* dof_body_ids, const int32_t* dof_offsets,
                                   int n_joints, float* gts, float* grs, float* lrs, float* grvs, float* gravs, float* dvs,
                                   void* stream) {
    ASE_CHECK_ARG(rotation && root_translation && root_velocity && root_angular_velocity && local_translation &&
                      parent_indices && clip_first && clip_num_frames && clip_fps && frame_clip && dof_body_ids &&
                      dof_offsets && gts && grs && lrs && grvs && gravs && dvs,
                  "clip_frames: null operand");
    ASE_CHECK_ARG(n_clips >= 1 && n_frames >= 2 * (int64_t)n_clips, "clip_frames: bad sizes (%d clips, %d frames; a clip has 2 or more)",
                  n_clips, n_frames);
    ASE_CHECK_ARG(n_bodies >= 1 && n_bodies <= kMaxClipBodies, "clip_frames: %d bodies (1-%d)", n_bodies, kMaxClipBodies);
    ASE_CHECK_ARG(n_joints >= 1 && n_joints <= kMaxClipJoints, "clip_frames: %d joints (1-%d)", n_joints, kMaxClipJoints);
    ASE_CHECK_ARG((int64_t)n_frames * (n_bodies + n_joints) < (int64_t)1 << 31, "clip_frames: %d frames are too many", n_frames);
    ClipFramesArgs a = {};
    ASE_CHECK_ARG(dof_offsets[0] == 0, "clip_frames: dof_offsets do not start at 0");
    for (int j = 0; j < n_joints; ++j) {
        const int sz = dof_offsets[j + 1] - dof_offsets[j];
        ASE_CHECK_ARG(sz == 1 || sz == 3, "clip_frames: joint %d has %d dofs (1 or 3 supported)", j, sz);
        ASE_CHECK_ARG(dof_body_ids[j] >= 0 && dof_body_ids[j] < n_bodies, "clip_frames: joint %d on body %d of %d", j,
                      dof_body_ids[j], n_bodies);
        a.dof_off[j] = dof_offsets[j];
        a.dof_body[j] = (uint8_t)dof_body_ids[j];
    }
    a.dof_off[n_joints] = dof_offsets[n_joints];
    // the ancestor chains: a parent precedes its child (poselib builds the global transforms in index order), -1 marks a root
    ASE_CHECK_ARG(parent_indices[0] == -1, "clip_frames: body 0 is not a root (parent %d)", parent_indices[0]);
    for (int b = 0; b < n_bodies; ++b) {
        const int p = parent_indices[b];
        ASE_CHECK_ARG(p >= -1 && p < b, "clip_frames: parent %d of body %d does not precede it", p, b);
        const int d = p < 0 ? 0 : a.depth[p] + 1;
        a.depth[b] = (uint8_t)d;
        for (int x = 0; x < d; ++x) a.chain[b][x] = a.chain[p][x];
        a.chain[b][d] = (uint8_t)b;
    }
    a.rot = rotation; a.root_t = root_translation; a.root_v = root_velocity; a.root_w = root_angular_velocity;
    a.local_t = local_translation; a.clip_first = clip_first; a.clip_frames = clip_num_frames; a.frame_clip = frame_clip;
    a.clip_fps = clip_fps;
    a.gts = gts; a.grs = grs; a.lrs = lrs; a.grvs = grvs; a.gravs = gravs; a.dvs = dvs;
    a.T = n_frames; a.C = n_clips; a.B = n_bodies; a.J = n_joints; a.D = dof_offsets[n_joints];
    const int64_t items = (int64_t)n_frames * (n_bodies + n_joints);
    ASE_LAUNCH(clip_frames_kernel, dim3((unsigned)((items + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, a);
    ASE_CHECK_LAUNCH("clip_frames");
    return ASE_OK;
}
