// The demo fetch of the AMP data path: HumanoidAMP.fetch_amp_obs_demo + build_amp_obs_demo
// (env/tasks/humanoid_amp.py:63-105 of the reference) as ONE launch over the (sample, history slot) items - the draws, the
// motion sampler, the frame builder and the store into the demo ring, no intermediate tensor in HBM.  The sampler and the frame
// builder are the device functions of amp_frames.h, the ones ase_hip_motion_state and ase_hip_build_amp_obs run, so the rows are
// bitwise those of the two-launch chain; the draws follow the table of ase_hip_amp_demo_fetch in include/ase_hip.h.
#include "amp_frames.h"
#include "philox.h"

namespace {

constexpr int kMaxSteps = 64;               // history slots: all slots of a sample sit in one block
constexpr int kItemsPerBlock = 32;          // (sample, slot) items a block aims at, as amp_reset.hip: 512 threads
constexpr int kLanesPerItem = 16;           // an item's joints, root and key bodies are spread over 16 lanes
constexpr int kMaxThreads = kMaxSteps * kLanesPerItem;
constexpr int kMaxFrame = 255;              // the widest frame ase_hip_build_amp_obs stages
constexpr int kMaxKeys = (kMaxFrame - 13 - 7) / 3;       // key bodies a frame of that width can hold beside one hinge

struct AmpDemoArgs {
    MotionClips c;                                           // (its key_body table is not used: key_body below)
    int key_body[kMaxKeys];
    const int32_t* motion_ids;                               // passed-in draws [n], or
    const float* times0;
    const uint64_t* rng;                                     // {seed, offset} and
    const uint32_t* cdf;                                     // [n_clips]: clip m is drawn for v in [cdf[m - 1], cdf[m])
    int32_t* motion_ids_out;                                 // the exported decisions, both or none
    float* times0_out;
    const int32_t* head_dev;                                 // nullable: added to head when the launch runs
    float* out;                                              // [ring_rows, ld_out]
    int64_t ld_out;
    float trunc, neg_dt;                                     // (float)(-dt)
    int n, n_clips, S, F, K, rows_per_block, ring_rows, head;
    int local_root, root_height;
};

// One lane per (item, part), as amp_reset_body: a motion state and a frame are ~200 dependent transcendental calls, one lane
// per item would make the launch as slow as that chain.  Lanes 0-14 of an item take its joints, lane 15 the root; key bodies
// and copies are spread over all 16.  Phase 0: the first lane of a sample reads or draws its clip and time into LDS; phase 1:
// the pose of every slot; phase 2: the frames.  LDS: per item a frame [F] and the sampler's scratch (dof positions [D], key
// body positions [3 K], root state [13]), pitch odd; then per sample of the block its clip (-1: skip the sample) and time.
__global__ __launch_bounds__(kMaxThreads) void amp_demo_fetch_kernel(AmpDemoArgs a) {
    extern __shared__ float tile[];
    const int F = a.F, S = a.S, D = a.c.D, K = a.K, J = a.c.J, R = a.rows_per_block;
    const int pitch = (F + D + 3 * K + 13) | 1;
    int* mid_s = (int*)(tile + R * S * pitch);
    float* time_s = (float*)(mid_s + R);
    const int tid = threadIdx.x;
    const int item = tid / kLanesPerItem, sub = tid - item * kLanesPerItem;
    const int r = item / S, s = item - r * S;                // the item's sample within the block and its history slot
    const int row = blockIdx.x * R + r;
    const bool live = r < R && row < a.n;
    // ---- phase 0
    if (live && s == 0 && sub == 0) {
        int mid;
        float t0;
        if (a.rng) {
            // the draw table of ase_hip_amp_demo_fetch: element 2 i + j of the stream is draw j of sample i
            const uint64_t seed = a.rng[0], off = a.rng[1], e2 = 2 * (uint64_t)row;
            // the first m with v < cdf[m]; cdf[n_clips - 1] = 2^24 > v
            const uint32_t v = philox_word<2>(seed, off, e2) >> 8;
            int lo = 0, hi = a.n_clips - 1;
            while (lo < hi) {
                const int m = (lo + hi) >> 1;
                if (v < a.cdf[m]) hi = m; else lo = m + 1;
            }
            mid = lo;
            t0 = philox_uniform(seed, off, e2 + 1) * (a.c.lengths[mid] - a.trunc) + a.trunc;
        } else {
            mid = a.motion_ids[row];
            t0 = a.times0[row];
        }
        if (a.motion_ids_out) { a.motion_ids_out[row] = mid; a.times0_out[row] = t0; }
        // a clip outside the library: the sample is skipped, never dereferenced
        mid_s[r] = mid >= 0 && mid < a.n_clips ? mid : -1;
        time_s[r] = t0;
    }
    __syncthreads();
    const int mid = live ? mid_s[r] : -1;
    const bool work = mid >= 0;
    float* o = tile + (work ? item : 0) * pitch;
    float* sdp = o + F;                                      // scratch: dof positions, key body positions, root state
    float* skp = sdp + D;
    float* srt = skp + 3 * K;
    const int od = 13 + 6 * J;
    // ---- phase 1: the pose k steps before the sampled time; the dof velocities, a copy of a clip row, go straight to their
    // columns of the frame
    if (work) {
        const FrameBlend fb = motion_blend(a.c, mid, time_s[r] + a.neg_dt * (float)s);
        if (sub == kLanesPerItem - 1) {
            motion_root(a.c, fb, srt, srt + 3, srt + 7, srt + 10);
        } else {
            for (int j = sub; j < J; j += kLanesPerItem - 1) motion_joint(a.c, fb, j, sdp, 1);
        }
        for (int d = sub; d < D; d += kLanesPerItem) o[od + d] = a.c.dvs[fb.f0 * D + d];
        for (int k = sub; k < K; k += kLanesPerItem) motion_body(a.c, fb, a.key_body[k], skp + 3 * k);
    }
    __syncthreads();
    // ---- phase 2: the frame of the scratch pose
    if (work) {
        const FrameDims dims{D, K, J, a.local_root, a.root_height};
        if (sub == kLanesPerItem - 1) {
            frame_root(dims, srt, srt + 3, srt + 7, srt + 10, o);
        } else {
            for (int j = sub; j < J; j += kLanesPerItem - 1) frame_joint(a.c.dof_off, j, sdp, 1, o);
        }
        if (sub < K) {
            const Q4 hq = heading_quat_inv(load_q(srt + 3));
            for (int k = sub; k < K; k += kLanesPerItem) frame_key(hq, srt, skp + 3 * k, o + od + D + 3 * k);
        }
    }
    __syncthreads();
    // samples leave row-contiguous: lanes walk the S F columns of every sample of the block, slot k at columns [k F, (k + 1) F)
    int64_t head = a.head;
    if (a.head_dev) {
        const int hd = *a.head_dev;
        if (hd < 0 || hd >= a.ring_rows) return;             // a head outside the ring: nothing is written
        head += hd;
    }
    const int rows = min(R, a.n - (int)blockIdx.x * R);
    for (int i = 0; i < rows; ++i) {
        if (mid_s[i] < 0) continue;
        float* h = a.out + ((head + (int64_t)blockIdx.x * R + i) % a.ring_rows) * a.ld_out;
        for (int x = tid; x < S * F; x += (int)blockDim.x) {
            const int sl = x / F, f = x - sl * F;
            h[x] = tile[(i * S + sl) * pitch + f];
        }
    }
}

}  // namespace

extern "C" int ase_hip_amp_demo_fetch(const float* gts, const float* grs, const float* lrs, const float* grvs, const float* gravs,
                                      const float* dvs, int n_bodies, const float* lengths, const int32_t* num_frames,
                                      const float* dt, const int32_t* length_starts, int n_clips, const int32_t* dof_body_ids,
                                      const int32_t* dof_offsets, int n_joints, const int32_t* key_body_ids, int n_key,
                                      const int32_t* motion_ids, const float* motion_times0, uint64_t* rng_state,
                                      const uint32_t* cdf, int advance, int32_t* motion_ids_out, float* motion_times0_out, int n,
                                      int n_steps, float truncate_time, float step_dt, int local_root_obs, int root_height_obs,
                                      float* out, int64_t ld_out, int ring_rows, int head, const int32_t* head_dev, void* stream) {
    ASE_CHECK_ARG(gts && grs && lrs && grvs && gravs && dvs && lengths && num_frames && dt && length_starts && dof_body_ids &&
                      dof_offsets && (key_body_ids || n_key == 0) && out,
                  "amp_demo_fetch: null operand");
    const bool given = motion_ids || motion_times0, drawn = rng_state || cdf;
    ASE_CHECK_ARG(given != drawn, "amp_demo_fetch: %s", given ? "passed-in draws (motion_ids, motion_times0) and device draws "
                  "(rng_state, cdf) at once" : "neither passed-in draws (motion_ids, motion_times0) nor device draws (rng_state, cdf)");
    ASE_CHECK_ARG(!given || (motion_ids && motion_times0), "amp_demo_fetch: passed-in draws need motion_ids and motion_times0");
    ASE_CHECK_ARG(!drawn || (rng_state && cdf), "amp_demo_fetch: device draws need rng_state and cdf");
    ASE_CHECK_ARG((motion_ids_out != nullptr) == (motion_times0_out != nullptr),
                  "amp_demo_fetch: the export (motion_ids_out, motion_times0_out) comes both or none");
    ASE_CHECK_ARG(n >= 1 && n_bodies >= 1 && n_clips >= 1, "amp_demo_fetch: bad sizes (n %d, bodies %d, clips %d)", n, n_bodies, n_clips);
    ASE_CHECK_ARG(n_steps >= 1 && n_steps <= kMaxSteps, "amp_demo_fetch: n_steps %d (1-%d history slots)", n_steps, kMaxSteps);
    ASE_CHECK_ARG(n_joints >= 1 && n_joints <= kMaxJoints && n_key >= 0 && n_key <= kMaxKeys,
                  "amp_demo_fetch: %d joints (1-%d), %d key bodies (at most %d)", n_joints, kMaxJoints, n_key, kMaxKeys);
    ASE_CHECK_ARG(ring_rows >= 1 && n <= ring_rows, "amp_demo_fetch: n %d does not fit a ring of %d rows", n, ring_rows);
    ASE_CHECK_ARG(head >= 0 && head < ring_rows, "amp_demo_fetch: head %d outside [0, %d)", head, ring_rows);
    AmpDemoArgs a = {};
    MotionClips& c = a.c;
    c.gts = gts; c.grs = grs; c.lrs = lrs; c.grvs = grvs; c.gravs = gravs; c.dvs = dvs;
    c.lengths = lengths; c.dt = dt; c.num_frames = num_frames; c.length_starts = length_starts;
    c.B = n_bodies; c.J = n_joints; c.K = 0; c.D = dof_offsets[n_joints];
    ASE_CHECK_ARG(dof_offsets[0] == 0 && c.D >= 1, "amp_demo_fetch: dof_offsets do not cover the dofs (first offset %d)", dof_offsets[0]);
    for (int j = 0; j <= n_joints; ++j) c.dof_off[j] = dof_offsets[j];
    for (int j = 0; j < n_joints; ++j) {
        const int sz = dof_offsets[j + 1] - dof_offsets[j];
        ASE_CHECK_ARG(sz == 1 || sz == 3, "amp_demo_fetch: joint %d has %d dofs (1 or 3 supported)", j, sz);
        ASE_CHECK_ARG(dof_body_ids[j] >= 0 && dof_body_ids[j] < n_bodies, "amp_demo_fetch: joint %d on body %d of %d", j,
                      dof_body_ids[j], n_bodies);
        c.dof_body[j] = dof_body_ids[j];
    }
    for (int k = 0; k < n_key; ++k) {
        ASE_CHECK_ARG(key_body_ids[k] >= 0 && key_body_ids[k] < n_bodies, "amp_demo_fetch: key body %d out of range", key_body_ids[k]);
        a.key_body[k] = key_body_ids[k];
    }
    a.F = 13 + 6 * n_joints + c.D + 3 * n_key;
    ASE_CHECK_ARG(a.F <= kMaxFrame, "amp_demo_fetch: frame of %d floats does not fit the staging tile (at most %d)", a.F, kMaxFrame);
    ASE_CHECK_ARG(ld_out >= (int64_t)n_steps * a.F, "amp_demo_fetch: ld_out %lld below n_steps * F = %d", (long long)ld_out,
                  n_steps * a.F);
    a.K = n_key; a.S = n_steps; a.n = n; a.n_clips = n_clips;
    a.rows_per_block = n_steps >= kItemsPerBlock ? 1 : kItemsPerBlock / n_steps;
    const int threads = (a.rows_per_block * n_steps * kLanesPerItem + 63) / 64 * 64;
    const int pitch = (a.F + c.D + 3 * n_key + 13) | 1;
    const int lds = (a.rows_per_block * n_steps * pitch + 2 * a.rows_per_block) * (int)sizeof(float);
    ASE_CHECK_ARG(lds <= 64 * 1024, "amp_demo_fetch: %d slots of a %d-float frame do not fit the staging tile", n_steps, a.F);
    ASE_CHECK_ARG(ring_rows >= 1 && n <= ring_rows, "amp_demo_fetch: n %d does not fit a ring of %d rows", n, ring_rows);
    ASE_CHECK_ARG(head >= 0 && head < ring_rows, "amp_demo_fetch: head %d outside [0, %d)", head, ring_rows);
    a.motion_ids = motion_ids; a.times0 = motion_times0; a.rng = rng_state; a.cdf = cdf;
    a.motion_ids_out = motion_ids_out; a.times0_out = motion_times0_out; a.head_dev = head_dev;
    a.out = out; a.ld_out = ld_out; a.trunc = truncate_time; a.neg_dt = -step_dt;
    a.ring_rows = ring_rows; a.head = head;
    a.local_root = local_root_obs != 0; a.root_height = root_height_obs != 0;
    ASE_LAUNCH(amp_demo_fetch_kernel, dim3((n + a.rows_per_block - 1) / a.rows_per_block), dim3(threads), lds, (hipStream_t)stream, a);
    if (drawn && advance) ASE_LAUNCH(rng_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, rng_state);   // a call is one stream position
    ASE_CHECK_LAUNCH("amp_demo_fetch");
    return ASE_OK;
}
